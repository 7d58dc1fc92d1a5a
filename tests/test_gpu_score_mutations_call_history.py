"""Call history of the mutational scan: on ONE long-lived model score_mutations (the cone and the dense route, "auto", with pairs)
is interleaved with score, score_sequences, conditional_probs and sample; every result equals a fresh model's on cloned inputs bit
for bit (tests/call_history.py).  The scan is attached to 'the NEXT namp_decoder_fwd call' of the thread: every plain call that
follows an attached one must be a plain call."""
import numpy as np
import pytest
import torch

import call_history as ch
from call_history import assert_same, make_model, step
from test_gpu_call_history import K_DUPLEX, L_DUPLEX, _duplex, cone, duplex_fd, sampler, score
from test_gpu_score_library_call_history import library, scorer

pytestmark = pytest.mark.gpu


def rna_positions():
    cx = _duplex()[0]
    return torch.from_numpy(np.nonzero((cx["mask"] * cx["chain_mask"] * cx["rna_mask"]) != 0)[0]).to(ch.DEV)


def scanner(pos, method, pairs=False):
    return lambda mo, f: mo.score_mutations(f, positions=pos, pairs=pairs, method=method)


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_score_mutations_in_a_call_history(weights_np, prec):
    """cone -> score -> dense -> conditional_probs -> active library -> cone -> auto with pairs -> paired conditional_probs -> cone ->
    sample -> cone -> score -> dense library -> dense -> sample: every step equals a fresh model's, repeated steps equal their
    first occurrence, and the cone and dense routes stay within 2e-4 per row of each other."""
    pairs = _duplex()[1]
    one, two = duplex_fd(bs=1), duplex_fd(bs=2)
    paired = dict(one, paired_residues=pairs)
    pos = rna_positions()
    lpos, ltok = library(5, 2)
    u = ch.uniforms(two, 8)
    m = make_model(weights_np, K_DUPLEX, precision=prec)
    a0 = step(m, scanner(pos, "cone"), one, "cone, first")
    assert a0["method"] == "cone" and not torch.isnan(a0["delta"]).any() and a0["delta"].shape == (len(pos), 4)
    s0 = step(m, score, one, "score after the cone")
    d0 = step(m, scanner(pos, "dense"), one, "dense")
    assert d0["method"] == "dense" and float((a0["delta"] - d0["delta"]).abs().max()) < 2e-4 * L_DUPLEX
    c0 = step(m, cone, one, "conditional_probs after dense")
    l0 = step(m, scorer(lpos, ltok, "active"), one, "active library after the scan")
    assert_same(step(m, scanner(pos, "cone"), one, "cone after the library"), a0, "cone, before and after the library")
    p0 = step(m, scanner(pos, "auto", True), paired, "auto with pairs")
    assert p0["sites"].shape[1] == 2 and p0["method"] == "cone"
    c1 = step(m, cone, paired, "conditional_probs with pairs")
    assert not torch.equal(c1["log_probs"], c0["log_probs"])
    assert_same(step(m, scanner(pos, "cone"), one, "cone after the paired calls"), a0, "cone, before and after the paired calls")
    draw = step(m, sampler(u), two, "sample after the cone")
    assert_same(step(m, scanner(pos, "cone"), one, "cone after sample"), a0, "cone, before and after sample")
    assert_same(step(m, score, one, "score after the cone, again"), s0, "score, before and after")
    step(m, scorer(lpos, ltok, "dense"), one, "dense library after the cone")
    assert_same(step(m, scanner(pos, "dense"), one, "dense, last"), d0, "dense, first and last")
    assert_same(step(m, scorer(lpos, ltok, "active"), one, "active library, last"), l0, "active library, before and after")
    assert_same(step(m, sampler(u), two, "sample, last"), draw, "sample, before and after")
    assert_same(step(m, cone, one, "conditional_probs, last"), c0, "conditional_probs, first and last")
    assert_same(step(m, scanner(pos, "auto", True), paired, "auto with pairs, last"), p0, "pairs, first and last")


def test_refused_mutation_calls_leave_nothing_behind(weights_np):
    """A token id 33 (IndexError), unsorted positions, a repeated residue and both forms at once (ValueError) are refused on the host
    before anything is attached: the calls that follow equal the fresh model's."""
    one = duplex_fd(bs=1)
    pos = rna_positions()
    m = make_model(weights_np, K_DUPLEX)
    a0 = step(m, scanner(pos, "cone"), one, "cone, first")
    with pytest.raises(IndexError):
        m.score_mutations(one, positions=pos, tokens=torch.tensor([26, 33]), method="cone")
    with pytest.raises(ValueError):
        m.score_mutations(one, positions=pos.flip(0), method="cone")
    with pytest.raises(ValueError):
        m.score_mutations(one, sites=torch.tensor([[51, 51]]), site_tokens=torch.tensor([[0, 26, 27]]), method="cone")
    with pytest.raises(ValueError):
        m.score_mutations(one, positions=pos, sites=torch.tensor([[51]]), site_tokens=torch.tensor([[0, 26]]))
    s0 = step(m, score, one, "score after the refused calls")
    assert_same(step(m, scanner(pos, "cone"), one, "cone after the refused calls"), a0, "cone, before and after")
    assert_same(step(m, score, one, "score, last"), s0, "score, before and after")
