"""Call history of the pair-class conditionals (ProteinMPNN.conditional_probs(classes=True)) on ONE long-lived model:
every result is compared bit for bit with a fresh model's on cloned inputs (tests/call_history.py) — the cached class tables, the
cached pair / group tables of the classes=False calls, the sampler's class tables and the thread's attachment do not leak."""
import pytest
import torch

import call_history as ch
import class_loo_ref as C

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

WOBBLE = ("paired_wobble", "paired_wobble_bias")
TIES = ("paired_residues", "paired_weights", "symmetry_residues", "symmetry_weights", "symmetry_token_maps") + WOBBLE


def to_dev(fd):
    return {k: (v.to(ch.DEV) if isinstance(v, torch.Tensor) else v) for k, v in fd.items()}


def without(keys):
    return lambda mo, f: mo.conditional_probs({k: v for k, v in f.items() if k not in keys})


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_call_history_with_class_calls(weights_np, prec):
    """plain -> classes pair call -> canonical pair call (the SAME resident feature_dict without the wobble keys) -> classes tied call
    with states -> sample() with wobble -> plain, and the classes pair call again: each the fresh model's bits, the first and the
    last plain call and the two class calls equal."""
    m = ch.make_model(weights_np, 16, precision=prec)
    fd_p = to_dev(C.case_inputs("l48_k16"))
    fd_s = to_dev(C.case_inputs("states_pairs"))
    u = ch.uniforms(fd_p, 3)
    classes_pair = lambda mo, f: mo.conditional_probs(f, classes=True)
    classes_tied = lambda mo, f: mo.conditional_probs(f, tied=True, classes=True)
    first = ch.step(m, without(TIES), fd_p, "plain")
    a = ch.step(m, classes_pair, fd_p, "classes pair call")
    canon = ch.step(m, without(WOBBLE), fd_p, "canonical pair call")
    ch.step(m, classes_tied, fd_s, "classes tied call with states")
    ch.step(m, lambda mo, f: mo._sample(f, mo.sample_level_walk, uniform=u), fd_p, "sample() with wobble")
    last = ch.step(m, without(TIES), fd_p, "plain again")
    ch.assert_same(last, first, "plain, first and last")
    ch.assert_same(ch.step(m, classes_pair, fd_p, "classes pair call again"), a, "classes pair call, first and last")
    assert "pair_class_log_probs" in a and "pair_class_log_probs" not in canon
    assert not torch.equal(a["log_probs"], canon["log_probs"]) and torch.equal(a["cone_items"], canon["cone_items"])
