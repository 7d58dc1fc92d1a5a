"""Call histories around the symmetric scan (ProteinMPNN.score_mutations(tied=True)): both routes interleaved with
score, the plain scan, score_tied(items), conditional_probs(tied=True) and a design call on ONE model; every result equals a fresh
model's on cloned inputs bit for bit (tests/call_history.py): no key, group table or attachment reaches a later call."""
import pytest
import torch

import call_history as CH
import group_scan_ref as GR
from tied_states_ref import to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def test_both_routes_between_the_other_calls(weights_np):
    c = GR.case("dimer_l48")
    fd = to_dev(c["fd"], CH.DEV)
    plain = {k: v for k, v in fd.items() if k not in ("symmetry_residues", "symmetry_weights")}
    plain.update(symmetry_residues=[[]], symmetry_weights=[[]])
    st, tk = torch.from_numpy(c["st"]), torch.from_numpy(c["tk"])
    lib = to_dev({"S": GR.reference("dimer_l48")["S"][:3]}, CH.DEV)["S"]
    u = CH.uniforms(fd, 3)
    m = CH.make_model(weights_np, c["K"])
    cone = lambda mo, f: mo.score_mutations(f, sites=st, site_tokens=tk, method="cone", tied=True)
    dense = lambda mo, f: mo.score_mutations(f, sites=st, site_tokens=tk, method="dense", tied=True)
    others = [("score", lambda mo, f: mo.score(f), plain),
              ("the plain scan", lambda mo, f: mo.score_mutations(f, positions=torch.tensor([0, 4, 9]), method="cone"), fd),
              ("score_tied(items)", lambda mo, f: mo.score_tied(f, lib, method="items"), fd),
              ("conditional_probs(tied)", lambda mo, f: mo.conditional_probs(f, tied=True), fd),
              ("sample", lambda mo, f: mo._sample(f, mo.sample_level_walk, uniform=u), fd)]
    first = CH.step(m, cone, fd, "the cone route, first call")
    for what, call, f in others:
        CH.step(m, call, f, what + " after a scan")               # (after the cone route first, after the dense route from then on)
        CH.step(m, cone, fd, "the cone route after " + what)
        CH.step(m, dense, fd, "the dense route after " + what)
    CH.assert_same(cone(m, fd), first, "the cone route at the end of the history")
