"""Call history of the coordinate gradients: the record of namp_train_feat_xgrad is thread state that "goes to the NEXT
call", the larger tile_ws and the gradient of X18 are per call.  On ONE long-lived model: a training step, a step with coordinate
gradients, score(), a training step without, a failed attach followed by a plain step — every result bit for bit that of a fresh model
(tests/call_history.py) with the weights of that moment on cloned inputs.  K = 16: the backward has no fp32 atomics (train.py:
gpa_tiles), so a training step repeats its own bits and the bar is torch.equal for every tensor."""
import pytest
import torch

from na_mpnn_amd import hip, train
import call_history as ch
from call_history import assert_same, make_model

pytestmark = pytest.mark.gpu


def test_steps_with_and_without_coordinate_gradients_on_one_model(weights_np):
    K = 16
    fd = ch.batch_fd([40, 33], seed=740, masked_frac=0.0)
    rm, rn, no_loss = ch.loss_tables()
    m = make_model(weights_np, K, train=True)
    opts = {}

    def train_call(mo, f):
        opt = opts.setdefault(id(mo), train.get_std_opt(mo.parameters(), 128, 0))
        with torch.enable_grad():
            loss, lp = train.train_step(mo, opt, f, rm, rn, no_loss, decoding_randn=f["randn"])
        return {"loss": loss, "log_probs": lp, "grads": [p.grad.clone() for p in mo.parameters()]}

    def xgrad_call(mo, f):
        return mo.coordinate_gradients(f)

    def score_call(mo, f):
        with torch.no_grad():
            return mo.score(f)

    def failed_attach_then_step(mo, f):
        assert hip.lib().namp_train_feat_xgrad(0) == -1            # NAMP_EINVAL: nothing stays attached
        return train_call(mo, f)

    def hist(call, what):
        f, ffd = ch.fresh(m), ch.fresh_fd(fd)                      # the weights of this moment: a training step moves them
        got = call(m, fd)
        assert_same(got, call(f, ffd), what)
        return got

    a = hist(train_call, "training step")
    x = hist(xgrad_call, "step with coordinate gradients")
    assert x["dX"].shape == fd["X"].shape and float(x["dX"].abs().max()) > 0
    hist(score_call, "score()")
    b = hist(train_call, "training step after the coordinate gradients")
    assert not torch.equal(a["loss"], b["loss"])                   # the optimiser has moved the weights in between
    hist(failed_attach_then_step, "failed attach, then a plain step")
    x2 = hist(xgrad_call, "coordinate gradients again")
    assert not torch.equal(x["dX"], x2["dX"])
