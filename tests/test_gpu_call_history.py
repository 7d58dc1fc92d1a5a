"""GPU tests of call HISTORIES: what one call leaves behind for the next on the same model object, the same library thread and the same
process — the packed weights, the V cache, the converted inputs, the token checks, the workspace, the pair tables (model.py); the
thread-local token maps / class tables / pair sections that "go to the NEXT call" (csrc); the step cache, the pack plan and the bf16
tiles shared by all models of the process (train.py); FusedAdam's host step count, plan and pointer ring.  Every result of the
long-lived model is compared bit for bit with a fresh model on cloned inputs (tests/call_history.py); one step per history is anchored
to the CPU oracle; histories that train compare parameters under the spread of four or more identical solo runs."""
import functools

import numpy as np
import pytest
import torch

from na_mpnn_amd import hip, synth, train
from oracle import cpu_ref
import call_history as ch
import real_structures as rs
import tied_states_ref
from call_history import DEV, RTI, assert_same, make_model, step

pytestmark = pytest.mark.gpu

score = lambda mo, f: mo.score(f)
cone = lambda mo, f: mo.conditional_probs(f, method="cone")


def sampler(u, walk=None):
    return lambda mo, f: mo._sample(f, mo.sample_level_walk if walk is None else walk, uniform=u)


# ------------------------------------------------------------------------------------------------------------------------------------
# b. precision modes in sequence
# ------------------------------------------------------------------------------------------------------------------------------------
def test_precision_modes_in_sequence(weights_np):
    """x3 -> fp32 -> bf16 -> (load_state_dict of other weights) -> x3 -> bf16 -> fp32 on one model and one resident fd: score after every
    switch equals a fresh model's in that mode."""
    fd = ch.design_fd(75, seed=710)
    m = make_model(weights_np, 24)
    other = {k: torch.from_numpy(v) for k, v in synth.make_weights(5).items()}
    seen = {}
    for i, prec in enumerate(("x3", "fp32", "bf16", "x3", "bf16", "fp32")):
        if i == 3:
            m.load_state_dict(other)
        m.message_precision = prec
        out = step(m, score, fd, f"score in mode {i} ({prec})")
        if i < 3:
            seen[prec] = out["log_probs"]
        else:
            assert not torch.equal(out["log_probs"], seen[prec])             # the new weights are the ones in use
        if i == 3:
            print(f"precision sequence: oracle max|dlogp| after load_state_dict (x3) = {ch.anchor_score(m, fd, out):.3e}")
    assert not torch.equal(seen["x3"], seen["fp32"]) and not torch.equal(seen["x3"], seen["bf16"])


# ------------------------------------------------------------------------------------------------------------------------------------
# c. shapes growing and shrinking
# ------------------------------------------------------------------------------------------------------------------------------------
def test_shapes_growing_and_shrinking(weights_np):
    """The model's one workspace grows and is then reused at every smaller shape: 2 x 120 (K = 30), 3 x 840 (K = 17: 2,520 residues,
    past the fused residue tail — the unfused path and the largest workspace), 1 x 17 (K = 16), 2 x 120 again; between them a sample and
    a cone conditional_probs on 90 residues, which allocate workspaces of their own."""
    assert 3 * 840 > hip.lib().namp_fused_tail_max_residues()
    small, big, tiny = ch.batch_fd([120, 120], seed=720), ch.batch_fd([840] * 3, seed=721), ch.batch_fd([17], seed=722)
    d90 = ch.design_fd(90, seed=723)
    u = ch.uniforms(d90, 4)
    m = make_model(weights_np, 30)
    first = step(m, score, small, "2 x 120")
    m.k_neighbors = 24
    step(m, sampler(u), d90, "sample on 90")
    m.k_neighbors = 17
    step(m, score, big, "3 x 840")
    grown = m._ws.numel()
    m.k_neighbors = 24
    step(m, cone, d90, "cone on 90")
    m.k_neighbors = 16
    step(m, score, tiny, "1 x 17")
    m.k_neighbors = 30
    again = step(m, score, small, "2 x 120 again")
    assert m._ws.numel() == grown                                             # (the shrinking calls did run in the grown workspace)
    assert_same(again, first, "2 x 120 before and after")
    print(f"growing and shrinking: oracle max|dlogp| at 2 x 120 = {ch.anchor_score(m, small, again):.3e}")


# ------------------------------------------------------------------------------------------------------------------------------------
# d / e / f: design calls on a 2 x 20 duplex beside a small protein
# ------------------------------------------------------------------------------------------------------------------------------------
L_DUPLEX, K_DUPLEX = 70, 24


@functools.lru_cache(maxsize=None)
def _duplex():
    """30 protein residues, a 20-nt DNA strand and the 20-nt RNA strand paired with it (a hybrid: G-U wobble may apply), as CPU data."""
    L = L_DUPLEX
    cx = synth.make_complex(seed=730, n=L, n_chains=3, frac_protein=30 / L, frac_dna=20 / L)
    assert int(cx["protein_mask"].sum()) == 30 and int(cx["dna_mask"].sum()) == 20 and int(cx["rna_mask"].sum()) == 20
    cx["chain_labels"] = np.repeat(np.arange(3, dtype=np.int32), (30, 20, 20))
    cx["R_idx"] = np.concatenate([np.arange(n, dtype=np.int32) + 100 * c for c, n in enumerate((30, 20, 20))])
    cx["chain_mask"][::9] = 0
    pairs = [(30 + i, 69 - i) for i in range(20)]
    bias = torch.zeros(1, L, 33)                                # synthetic weights know no chemistry (see paired_ref.make_case)
    for i in range(30, L):
        allowed = [RTI[n] for n in (("DA", "DC", "DG", "DT") if cx["dna_mask"][i] else ("A", "C", "G", "U"))]
        bias[0, i] = -1e8
        bias[0, i, allowed] = 0.0
    return cx, pairs, bias


def duplex_fd(bs=2, **extra):
    cx, pairs, bias = _duplex()
    fd = rs.sample_fd(cx, bs, 0.5, 731, bias=bias.clone())
    fd.update(extra)
    return rs.to_dev(fd, DEV)


def states_fd(bs=2):
    cx = _duplex()[0]
    randn = np.random.default_rng(732).standard_normal((bs, L_DUPLEX)).astype(np.float32)
    fd = tied_states_ref.states_fd(cx, tied_states_ref.make_states(cx, 2, seed=733), (0.6, 0.4), bs, 0.5, randn)
    return rs.to_dev(fd, DEV)


@pytest.mark.parametrize("walk", [True, False], ids=["walk", "per-level"])
def test_thread_local_tables_do_not_leak(weights_np, walk):
    """The token maps, class tables and pair sections go to 'the NEXT call' of the thread: every plain call that follows a mapped one
    must be a plain call.  paired -> plain -> wobble -> canonical paired -> plain -> two states -> plain -> cone with pairs -> cone
    without, in the persistent walk and in the per-level form (which attach the maps at different points of sample())."""
    pairs = _duplex()[1]
    plain, paired = duplex_fd(), duplex_fd(paired_residues=pairs)
    wobble = duplex_fd(paired_residues=pairs, paired_wobble=True, paired_wobble_bias=1.0)
    states = states_fd()
    u = ch.uniforms(plain, 5)
    m = make_model(weights_np, K_DUPLEX)
    draw = sampler(u, walk)
    base = step(m, draw, plain, "plain sample, first")
    tied = step(m, draw, paired, "paired sample")
    assert not torch.equal(tied["S"], base["S"])                              # (the maps do reach the kernel)
    for name, fd in (("plain after paired", plain), ("wobble", wobble), ("canonical after wobble", paired), ("plain after wobble", plain),
                     ("two states", states), ("plain after states", plain)):
        out = step(m, draw, fd, name)
        if fd is plain:
            assert_same(out, base, name + " against the first plain call")
        if fd is paired:
            assert_same(out, tied, name + " against the first paired call")
    one = duplex_fd(bs=1)
    c0 = step(m, cone, one, "cone without pairs, first")
    c1 = step(m, cone, dict(one, paired_residues=pairs), "cone with pairs")
    assert not torch.equal(c1["log_probs"], c0["log_probs"])
    assert_same(step(m, cone, one, "cone after pairs"), c0, "cone without pairs, before and after")
    assert_same(step(m, draw, plain, "plain sample after the cones"), base, "plain sample, last")
    assert m.sample_walk_status() == 0
    print(f"thread-local tables ({'walk' if walk else 'per-level'}): oracle max|dlogp| = {ch.anchor_score(m, one):.3e}")


def test_refused_calls_leave_nothing_behind(weights_np):
    """Host-side refusals in the middle of a history — a token id 33 (IndexError), a pair outside [0, L) (ValueError), paired_wobble in
    conditional_probs (NotImplementedError): the valid call of the same path and then a different path equal the fresh model's."""
    pairs = _duplex()[1]
    plain, one = duplex_fd(), duplex_fd(bs=1)
    u = ch.uniforms(plain, 6)
    m = make_model(weights_np, K_DUPLEX)
    step(m, score, one, "score, first")
    bad = dict(one, S=one["S"].clone())
    bad["S"][0, 7] = 33
    with pytest.raises(IndexError):
        m.score(bad)
    step(m, score, one, "score after the refused score")
    step(m, sampler(u), plain, "sample after the refused score")
    with pytest.raises(ValueError, match="outside"):
        m._sample(dict(plain, paired_residues=pairs[:3] + [(40, L_DUPLEX)]), True, uniform=u)
    step(m, sampler(u), dict(plain, paired_residues=pairs), "paired sample after the refused sample")
    step(m, sampler(u), plain, "plain sample after the refused sample")
    step(m, cone, one, "cone after the refused sample")
    with pytest.raises(NotImplementedError):
        m.conditional_probs(dict(one, paired_residues=pairs, paired_wobble=True), method="cone")
    step(m, cone, dict(one, paired_residues=pairs), "paired cone after the refused cone")
    got = step(m, score, one, "score after the refused cone")
    print(f"refused calls: oracle max|dlogp| = {ch.anchor_score(m, one, got):.3e}")


def test_in_place_edits_reach_the_caches(weights_np):
    """In-place edits of resident inputs between two calls: S.copy_, mask[0, 5] = 0 and X.add_ between two score() calls; mask and the
    dna / rna flags between two paired conditional_probs calls, where the pair tables and the host lists must be dropped."""
    pairs = _duplex()[1]
    fd = duplex_fd(bs=1)
    m = make_model(weights_np, K_DUPLEX)
    first = step(m, score, fd, "score, first")
    fd["S"].copy_(torch.roll(fd["S"], 1, 1).where(fd["protein_mask"].bool() & torch.roll(fd["protein_mask"], 1, 1).bool(), fd["S"]))
    fd["mask"][0, 5] = 0
    fd["X"].add_(0.25 * torch.randn(fd["X"].shape, generator=torch.Generator().manual_seed(7)).to(DEV) * fd["X_m"][..., None])
    second = step(m, score, fd, "score after the edits")
    assert not torch.equal(second["log_probs"], first["log_probs"])
    print(f"in-place edits: oracle max|dlogp| after the edits = {ch.anchor_score(m, fd, second):.3e}")
    pfd = dict(fd, paired_residues=pairs)
    c0 = step(m, cone, pfd, "paired cone, first")
    assert c0["pairs"].shape[0] == 20
    tables, lists = m._tie_tables[(False, False)][2], {k: m._tokens_ok[("host", k)][2] for k in ("dna_mask", "rna_mask", "mask")}
    assert step(m, cone, pfd, "paired cone, unchanged")["pairs"].shape[0] == 20 and m._tie_tables[(False, False)][2] is tables     # (the cache does hit)
    i, j = pairs[4]
    pfd["mask"][0, i] = 0                                                    # this pair is no longer tied
    a, _ = pairs[9]                                                          # a DNA member becomes an RNA residue: another token map
    assert int(pfd["dna_mask"][0, a]) == 1
    pfd["dna_mask"][0, a] = 0
    pfd["rna_mask"][0, a] = 1
    c1 = step(m, cone, pfd, "paired cone after the edits")
    assert m._tie_tables[(False, False)][2] is not tables
    assert all(m._tokens_ok[("host", k)][2] is not v for k, v in lists.items())
    assert c1["pairs"].shape[0] == 19 and [i, j] not in c1["pairs"].tolist()
    assert not torch.equal(c1["log_probs"][0, a], c0["log_probs"][0, a])


# ------------------------------------------------------------------------------------------------------------------------------------
# g / h / i: training histories
# ------------------------------------------------------------------------------------------------------------------------------------
def _batches():
    return ch.batch_fd([40, 33], seed=740, masked_frac=0.0), ch.batch_fd([37, 29], seed=741, masked_frac=0.0)


def _train(m, opt, fd, tables, **kw):
    rm, rn, no_loss = tables
    with torch.enable_grad():
        return train.train_step(m, opt, fd, rm, rn, no_loss, gradient_norm=1.0, decoding_randn=fd["randn"], **kw)


@pytest.mark.parametrize("K", [17, 16])
def test_two_models_share_the_training_globals(weights_np, K):
    """A (x3) and B (bf16, mixed precision) from the same weights, trained alternately A, B, A, B on the same two batches, against each
    trained alone: the step cache, the pack plan and the bf16 tiles are module globals shared by both.  Alternation thrashes the pack
    plan (each model's second step finds its blocks dropped by the other's step; a solo second step finds them all: both asserted);
    parameters agree under the spread of six identical solo runs, three before and three after the alternation
    (call_history.assert_within_spread).  K = 16: no atomics in the backward, the rule is an equality.  K = 17: fp32 atomics, a few
    discrete outcomes; the measured populations are in DESIGN §2, "Call histories"."""
    tables, batches = ch.loss_tables(), _batches()

    def new(prec):
        m = make_model(weights_np, K, train=True, precision=prec)
        return m, train.get_std_opt(m.parameters(), 128, 0)

    solo = {"x3": [], "bf16": []}

    def solo_runs(n):
        for _ in range(n):
            for prec in solo:
                m, opt = new(prec)
                for s, fd in enumerate(batches):
                    _train(m, opt, fd, tables)
                    # alone, the second step finds every block it asks for in the plan: nothing is registered again
                    assert train._PLAN.entries and train._PLAN.dirty == (s == 0), (prec, s)
                solo[prec].append(ch.flat_params(m))

    solo_runs(3)
    (A, optA), (B, optB) = new("x3"), new("bf16")
    for s, fd in enumerate(batches):
        for m, opt in ((A, optA), (B, optB)):
            _train(m, opt, fd, tables)
            if s == 1:      # begin_step dropped this model's blocks (the other model's step did not ask for them): packed singly, registered again
                assert train._PLAN.entries and train._PLAN.dirty
    pA, pB = ch.flat_params(A), ch.flat_params(B)
    assert train.X3 == 2                                                      # the module-level precision is B's, the last to run
    solo_runs(3)
    ch.assert_within_spread(pA, solo["x3"], f"K = {K}: alternating, model A (x3)")
    ch.assert_within_spread(pB, solo["bf16"], f"K = {K}: alternating, model B (bf16)")
    assert not torch.equal(solo["x3"][0], solo["bf16"][0])


@functools.lru_cache(maxsize=None)
def _oracle_gradients():
    """fp64 autograd of the oracle on the two micro-batches -> {name: g1 + g2}."""
    w = cpu_ref.to_dtype(cpu_ref.to_torch(synth.make_weights(0)), torch.float64)
    total = None
    for fd in _batches():
        fd_c = cpu_ref.to_dtype({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in fd.items()}, torch.float64)
        _, _, g = cpu_ref.train_loss_and_grads(w, fd_c, 17, fd_c["randn"], RTI)
        total = g if total is None else {k: total[k] + g[k] for k in g}
    return total


@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_gradient_accumulation(weights_np, prec):
    """forward_train + loss + backward on micro-batch 1, then on micro-batch 2 with no zero_grad between, against the sum of the two
    gradients computed separately; and forward_train twice, then ONE (loss1 + loss2).backward() — the first forward's backward then
    runs when its step is no longer the cache's step.  Bar: 5e-5 of the tensor's largest entry (the memory contract's bar for
    atomically accumulated gradients); the accumulated gradient against the oracle's fp64 autograd at the project's 2e-4."""
    rm, rn, no_loss = ch.loss_tables()
    mb = _batches()
    m = make_model(weights_np, 17, train=True, precision=prec)
    params = dict(m.named_parameters())

    def loss_of(fd):
        S, mfl = train._mask_for_loss(fd, no_loss)
        lp, _ = train.forward_train(m, fd, fd["randn"])
        pm = {"protein": fd["protein_mask"], "dna": fd["dna_mask"], "rna": fd["rna_mask"]}
        return train.loss_smoothed(S, lp, mfl, pm, rm, rn, num_letters=33)[1]

    def grads(*groups):
        """Each group of micro-batches: forwards, then one backward of the summed loss; no zero_grad between the groups."""
        m.zero_grad(set_to_none=True)
        with torch.enable_grad():
            for group in groups:
                sum(loss_of(fd) for fd in group).backward()
        return {n: p.grad.detach().clone() for n, p in params.items()}

    g1, g1b, g2 = grads([mb[0]]), grads([mb[0]]), grads([mb[1]])
    want = {n: g1[n] + g2[n] for n in g1}
    forms = {"two backwards, no zero_grad": grads([mb[0]], [mb[1]]), "two forwards, one backward": grads([mb[0], mb[1]])}
    spread = max(float((g1[n] - g1b[n]).abs().max()) / (float(g1[n].abs().max()) + 1e-30) for n in g1)
    print(f"gradient accumulation ({prec}): relative spread of two identical backward passes {spread:.3e}")
    ref = _oracle_gradients()
    for what, got in forms.items():
        worst = worst_ref = 0.0
        for n in want:
            scale = float(want[n].abs().max())
            d = float((got[n] - want[n]).abs().max())
            r, rscale = ref[n].to(DEV), float(ref[n].abs().max())
            dr = float((got[n].double() - r).abs().max())
            if rscale < 1e-12:
                assert float(got[n].abs().max()) < 1e-9, (what, n)
                continue
            worst, worst_ref = max(worst, d / scale), max(worst_ref, dr / rscale)
            assert d <= 5e-5 * scale, (what, n, d / scale)
            assert dr < 2e-4 * rscale, (what, n, dr / rscale)
        print(f"gradient accumulation ({prec}), {what}: worst {worst:.3e} of the largest entry against the separate sum, "
              f"{worst_ref:.3e} against the oracle's fp64 autograd")


@pytest.mark.parametrize("K", [17, 16])
def test_optimiser_state_through_a_checkpoint(tmp_path, weights_np, K):
    """(K = 16: no atomics in the backward, bit-reproducible training — the resumed run must equal the uninterrupted one to the bit.)
    Three fused steps, save_checkpoint, load_checkpoint into a NEW model with a NEW get_std_opt, two more steps, against five
    uninterrupted steps (same batches): the host-side step count, the moments and the Noam step survive.  Before the fifth step both arms
    keep the fourth step's gradient tensors alive across zero_grad, so the new gradients land at new addresses and the pointer table
    must be uploaded again."""
    tables, batches = ch.loss_tables(), _batches()
    path = str(tmp_path / "history.pt")

    def run(interrupted):
        m = make_model(weights_np, K, train=True)
        opt = train.get_std_opt(m.parameters(), 128, 0)
        for s in range(5):
            if s == 3 and interrupted:
                train.save_checkpoint(path, m, opt, epoch=0, step=opt._step)
                m = make_model(synth.make_weights(5), K, train=True)
                opt = train.get_std_opt(m.parameters(), 128, 0)
                train.load_checkpoint(path, m, opt, map_location=DEV)
                assert opt._step == 3
            keep, key = None, getattr(opt.optimizer, "_ptr_key", None)
            if s == 4:
                keep = [p.grad for p in m.parameters()]                      # alive across zero_grad: the allocator cannot hand them back
                assert all(g is not None for g in keep)
            _train(m, opt, batches[s % 2], tables)
            if s == 4:
                assert opt.optimizer._ptr_key != key and all(p.grad is not g for p, g in zip(m.parameters(), keep))
            del keep
        assert opt._step == 5 and opt.optimizer._t == 5
        assert all(float(opt.optimizer.state[p]["step"]) == 5.0 for p in m.parameters())
        return ch.flat_params(m)

    a, b, c, d, e = run(False), run(False), run(True), run(False), run(False)      # (the interrupted arm between the solo runs)
    ch.assert_within_spread(c, [a, b, d, e], f"K = {K}: three steps, checkpoint, two steps against five steps")
