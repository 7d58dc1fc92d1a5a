"""Call history of the forbidden motifs (ProteinMPNN.sample with feature_dict["forbidden_motifs"]) on ONE long-lived
model: motif calls interleaved with plain, paired and pair-terms sample(), score() and score_tied(method="sampler"); every result is
compared bit for bit with a fresh model's on cloned inputs (tests/call_history.py) — the section of one call, its larger workspace and
the thread's attachment do not reach the calls behind it."""
import pytest
import torch

import call_history as ch
import pair_terms_ref
from na_mpnn_amd import hip, spec
from paired_ref import make_case, to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TIES = ("paired_residues", "pair_terms", "forbidden_motifs")


def without(keys, call):
    return lambda mo, f: call(mo, {k: v for k, v in f.items() if k not in keys})


def test_call_history_with_motifs(weights_np):
    """motif call (with base pairs and pair terms) -> plain sample -> motif call alone -> paired sample -> pair-terms sample -> score ->
    score_tied by the sampler -> the first call again; a refused motif call and a refused attach leave nothing behind."""
    m = ch.make_model(weights_np, 24)
    L, bs = 60, 2
    rti = spec.restype_to_int()
    cx, fd_cpu, pairs = make_case(L, bs, 0.5, 8, seed=3100 + L)
    AA = torch.randn(33, 33, generator=torch.Generator().manual_seed(1))
    fd_cpu["pair_terms"] = pair_terms_ref.neighbour_terms(L, AA, "all", cx["chain_labels"].tolist())
    fd_cpu["forbidden_motifs"] = [(rti[n],) * 2 for n in ("DA", "DC", "DG", "DT", "A", "C", "G", "U")] + [(rti["ALA"], rti["LEU"], rti["ALA"])]
    fd = to_dev(fd_cpu, ch.DEV)
    u = ch.uniforms(fd, 3)
    sample = lambda mo, f: mo._sample(f, mo.sample_level_walk, uniform=u)
    first = ch.step(m, sample, fd, "motifs + pairs + pair terms")
    plain = ch.step(m, without(TIES, sample), fd, "plain sample")
    alone = ch.step(m, without(TIES[:2], sample), fd, "motifs alone")
    paired = ch.step(m, without(TIES[1:], sample), fd, "paired sample")
    terms = ch.step(m, without(("forbidden_motifs",), sample), fd, "pairs + pair terms")
    ch.step(m, without(TIES, lambda mo, f: mo.score(dict(f, batch_size=1, randn=f["randn"][:1]))), fd, "score")
    ch.step(m, without(TIES[1:], lambda mo, f: mo.score_tied(dict(f, randn=f["randn"][:1]), first["S"][:1], method="sampler")), fd,
            "score_tied by the sampler")
    ch.assert_same(ch.step(m, sample, fd, "motifs + pairs + pair terms again"), first, "motif call, first and last")
    assert int(first["motif_hits"].sum()) == 0 and int(alone["motif_hits"].sum()) == 0
    assert not torch.equal(first["sampling_probs"], terms["sampling_probs"]) and not torch.equal(alone["S"], plain["S"])
    assert "motif_hits" not in plain and "motif_hits" not in paired and "motif_hits" not in terms
    # a call the model refuses (a motif of one token) attaches nothing, and neither does a refused attach: the next call is the plain call
    with pytest.raises(ValueError, match="2..8"):
        m.sample(dict(fd, forbidden_motifs=[(1,)]))
    assert hip.lib().namp_sample_motifs(4, 9) == -1
    ch.assert_same(ch.step(m, without(TIES, sample), fd, "plain sample after a failed motif call"), plain, "plain sample, again")
