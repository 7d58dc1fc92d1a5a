"""Call histories around the paired scan (ProteinMPNN.score_mutations(tied=True, classes=True)): both routes
interleaved with score, the plain, state and group scans, score_tied(items), paired sample() and conditional_probs(classes=True) on ONE
model; every result equals a fresh model's on cloned inputs bit for bit (tests/call_history.py): no key, class table or attachment
reaches a later call."""
import pytest
import torch

import call_history as CH
import class_scan_ref as CR
import group_scan_ref as GR
import state_scan_ref as SR
from tied_states_ref import to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def test_both_routes_between_the_other_calls(weights_np):
    c = CR.case("l48_k16")
    fd = to_dev(c["fd"], CH.DEV)
    ties = ("paired_residues", "paired_weights", "paired_wobble", "paired_wobble_bias", "symmetry_residues", "symmetry_weights")
    plain = {k: v for k, v in fd.items() if k not in ties}
    plain.update(symmetry_residues=[[]], symmetry_weights=[[]])
    st, tk = torch.from_numpy(c["st"]), torch.from_numpy(c["tk"])
    lib = to_dev({"S": CR.reference("l48_k16")["S"][:3]}, CH.DEV)["S"]
    g = GR.case("dimer_l48")
    assert g["K"] == c["K"] == 16
    fd_g, st_g, tk_g = to_dev(g["fd"], CH.DEV), torch.from_numpy(g["st"]), torch.from_numpy(g["tk"])
    _, fd_s, K_s, sites_s, tks_s = SR.case("plain")
    assert K_s == 16
    fd_s, sites_s, tks_s = to_dev(fd_s, CH.DEV), torch.from_numpy(sites_s), torch.from_numpy(tks_s)
    u = CH.uniforms(fd, 3)
    m = CH.make_model(weights_np, c["K"])
    cone = lambda mo, f: mo.score_mutations(f, sites=st, site_tokens=tk, method="cone", tied=True, classes=True)
    dense = lambda mo, f: mo.score_mutations(f, sites=st, site_tokens=tk, method="dense", tied=True, classes=True)
    others = [("score", lambda mo, f: mo.score(f), plain),
              ("the plain scan", lambda mo, f: mo.score_mutations(f, positions=torch.tensor([0, 4, 9]), method="cone"), plain),
              ("the state scan", lambda mo, f: mo.score_mutations(f, sites=sites_s, site_tokens=tks_s, method="cone"), fd_s),
              ("the group scan", lambda mo, f: mo.score_mutations(f, sites=st_g, site_tokens=tk_g, method="cone", tied=True), fd_g),
              ("score_tied(items)", lambda mo, f: mo.score_tied(f, lib, method="items"), fd),
              ("conditional_probs(classes)", lambda mo, f: mo.conditional_probs(f, classes=True), fd),
              ("paired sample", lambda mo, f: mo._sample(f, mo.sample_level_walk, uniform=u), fd)]
    first = CH.step(m, cone, fd, "the cone route, first call")
    for what, call, f in others:
        CH.step(m, call, f, what + " after a scan")               # (after the cone route first, after the dense route from then on)
        CH.step(m, cone, fd, "the cone route after " + what)
        CH.step(m, dense, fd, "the dense route after " + what)
    CH.assert_same(cone(m, fd), first, "the cone route at the end of the history")
