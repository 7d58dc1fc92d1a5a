"""Call history of the compact pair terms (ProteinMPNN.sample with feature_dict["pair_terms"]) on ONE long-lived
model: every result is compared bit for bit with a fresh model's on cloned inputs (tests/call_history.py) — the section of one call,
its larger workspace and the thread's attachment do not reach the calls behind it."""
import pytest
import torch

import call_history as ch
import pair_terms_ref
from na_mpnn_amd import hip
from paired_ref import make_case, to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TIES = ("paired_residues", "pair_terms")


def without(keys, call):
    return lambda mo, f: call(mo, {k: v for k, v in f.items() if k not in keys})


def test_call_history_with_pair_terms(weights_np):
    """pair-terms call (with base pairs) -> plain sample -> paired sample -> score -> conditional_probs, each the fresh model's bits;
    the pair-terms call again gives its first result; a failed pair-terms call (65 slots) leaves no attachment behind."""
    m = ch.make_model(weights_np, 24)
    L, bs = 60, 2
    cx, fd_cpu, pairs = make_case(L, bs, 0.5, 8, seed=3100 + L)
    AA = torch.randn(33, 33, generator=torch.Generator().manual_seed(1))
    fd_cpu["pair_terms"] = pair_terms_ref.neighbour_terms(L, AA, "all", cx["chain_labels"].tolist())
    fd = to_dev(fd_cpu, ch.DEV)
    u = ch.uniforms(fd, 3)
    sample = lambda mo, f: mo._sample(f, mo.sample_level_walk, uniform=u)
    first = ch.step(m, sample, fd, "pair-terms call")
    plain = ch.step(m, without(TIES, sample), fd, "plain sample")
    paired = ch.step(m, without(("pair_terms",), sample), fd, "paired sample")
    ch.step(m, without(TIES, lambda mo, f: mo.score(dict(f, batch_size=1, randn=f["randn"][:1]))), fd, "score")
    ch.step(m, without(TIES, lambda mo, f: mo.conditional_probs(dict(f, randn=f["randn"][:1]))), fd, "conditional_probs")
    ch.assert_same(ch.step(m, sample, fd, "pair-terms call again"), first, "pair-terms call, first and last")
    assert not torch.equal(first["sampling_probs"], paired["sampling_probs"]) and not torch.equal(paired["S"], plain["S"])
    # a call the model refuses (65 slots) attaches nothing, and neither does a refused attach: the next call is the plain call
    bad = dict(fd, pair_terms=dict(fd["pair_terms"], partner=torch.full((1, L, 65), -1), table=torch.zeros(1, L, 65, dtype=torch.int64)))
    with pytest.raises(ValueError, match="slots"):
        m.sample(bad)
    assert hip.lib().namp_sample_pair_terms(65, 1, 0) == -1
    ch.assert_same(ch.step(m, without(TIES, sample), fd, "plain sample after a failed pair-terms call"), plain, "plain sample, again")
