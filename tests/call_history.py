"""Call histories: sequences of calls on ONE long-lived model object, every result checked against a FRESH model — same constructor
arguments, same weights at that moment, empty caches — on cloned inputs.  The inference entry points are bit-reproducible (DESIGN §2,
"Memory contract": the only buffers that are not are the training table gradients), so the bar is torch.equal; one step per history
is also anchored to the CPU oracle at the project's bars (1e-3 on log-probs, arg-max outside near ties as real_structures defines
them).  Helper module of test_gpu_call_history.py (not a test)."""
import torch

from na_mpnn_amd import spec, synth
from na_mpnn_amd.model import ProteinMPNN
from oracle import cpu_ref
import real_structures as rs

DEV = "cuda:0"
RTI = spec.restype_to_int()
# attributes a test may set on the instance and the fresh model must share
SWITCHES = ("message_precision", "k_neighbors", "reference_sample_mask_quirk", "sample_level_parallel", "sample_level_walk",
            "sample_check_walk", "sample_split_groups", "sample_pairs_device_plan", "loo_dense_tokens")


def make_model(weights_np, k, dropout=0.0, train=False, precision="x3"):
    m = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=k, dropout=dropout, atom_dict=spec.atom_dict(), restype_to_int=RTI,
                    polytype_to_int=spec.polytype_to_int())
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in weights_np.items()})
    m = m.to(DEV)
    m.message_precision = precision
    return m.train() if train else m.eval()


def fresh(m):
    """A new ProteinMPNN with m's constructor arguments, a clone of m.state_dict() taken NOW, m's switches and mode, empty caches."""
    polytypes = spec.polytype_to_int()
    assert m.features.node_embedding.weight.shape[1] == len(polytypes)
    f = ProteinMPNN(num_letters=m.num_letters, vocab=m.vocab, k_neighbors=m.k_neighbors, num_encoder_layers=len(m.encoder_layers),
                    num_decoder_layers=len(m.decoder_layers), dropout=m.dropout.p, atom_dict=m.atom_dict, restype_to_int=m.restype_to_int,
                    polytype_to_int=polytypes, protein_augment_eps=m.protein_augment_eps, dna_augment_eps=m.dna_augment_eps,
                    rna_augment_eps=m.rna_augment_eps, decode_protein_first=m.decode_protein_first, na_ref_atom=m.na_ref_atom,
                    include_pred_na_N=m.include_pred_na_N)
    f.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
    f = f.to(next(m.parameters()).device)
    for name in SWITCHES:
        if name in m.__dict__:
            setattr(f, name, m.__dict__[name])
    f.train(m.training)
    assert f._packed is None and f._v_cache is None and not f._conv and not f._tokens_ok and f._ws is None
    return f


def fresh_fd(fd):
    """Every tensor of the feature dict cloned: no identity-keyed cache can hit."""
    return {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in fd.items()}


def assert_same(got, ref, what):
    """Two results of the same entry point, bit for bit: tensors, tuples / dicts of tensors; other values by ==."""
    if torch.is_tensor(ref):
        assert torch.is_tensor(got) and got.shape == ref.shape and got.dtype == ref.dtype, what
        if not torch.equal(got, ref):
            d = (got.double() - ref.double()).abs()
            raise AssertionError(f"{what}: differs from the fresh model's result in {int((got != ref).sum())} of {ref.numel()} entries, "
                                 f"max |d| = {float(d.max()):.3e}")
    elif isinstance(ref, dict):
        assert set(got) == set(ref), (what, set(got) ^ set(ref))
        for k in ref:
            assert_same(got[k], ref[k], f"{what}[{k!r}]")
    elif isinstance(ref, (tuple, list)):
        assert len(got) == len(ref), what
        for i, (a, b) in enumerate(zip(got, ref)):
            assert_same(a, b, f"{what}[{i}]")
    else:
        assert got == ref, (what, got, ref)


def step(m, call, fd, what):
    """One step of a history: `call(model, fd)` on the long-lived model and the resident fd, then on a fresh model and cloned inputs;
    returns the long-lived model's result."""
    with torch.no_grad():
        got = call(m, fd)
        ref = call(fresh(m), fresh_fd(fd))
    assert_same(got, ref, what)
    return got


def batch_fd(ns, seed, dev=DEV, masked_frac=0.05):
    """A padded batch of synth complexes as a resident feature dict that every entry point takes (training keys and design keys)."""
    from na_mpnn_amd import shard
    cxs = [synth.make_complex(seed=seed + 10 * i + n, n=n, n_chains=min(3, n), masked_frac=masked_frac if n > 20 else 0.0)
           for i, n in enumerate(ns)]
    fd = shard.pad_batch(cxs)
    fd["S"] = fd["S"].long()
    B, L = fd["S"].shape
    fd["bias"] = torch.zeros(B, L, 33)
    fd = {k: v.to(dev) for k, v in fd.items()}
    fd.update(batch_size=1, temperature=0.5, symmetry_residues=[[]], symmetry_weights=[[]])
    return fd


def design_fd(n, seed, bs=1, dev=DEV, masked_frac=0.03):
    cx = synth.make_complex(seed=seed, n=n, masked_frac=masked_frac)
    cx["chain_mask"][::9] = 0
    fd = rs.sample_fd(cx, bs, 0.5, seed + 1)
    return rs.to_dev(fd, dev)


def uniforms(fd, seed):
    B_dec = fd["S"].shape[0] * fd["batch_size"]
    return torch.rand(B_dec, fd["S"].shape[1], generator=torch.Generator().manual_seed(seed)).to(fd["S"].device)


def anchor_score(m, fd, got=None):
    """score() of the long-lived model against the CPU oracle (evaluated in fp64) on the model's CURRENT state_dict: 1e-3 on the
    log-probs of unmasked residues, arg-max equal wherever the oracle's top two are at least NEAR_TIE apart (which, as on the real
    structures, may leave out at most MAX_LEFT_OUT of the rows, and one row).  Returns the largest difference."""
    with torch.no_grad():
        got = m.score(fd) if got is None else got
    w = cpu_ref.to_dtype({k: v.detach().cpu() for k, v in m.state_dict().items()}, torch.float64)
    fd_c = cpu_ref.to_dtype({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in fd.items()}, torch.float64)
    with torch.no_grad():
        ref = cpu_ref.score(w, fd_c, int(m.k_neighbors))["log_probs"]
    lp = got["log_probs"].cpu()
    valid = fd_c["mask"].bool()
    d = float((lp.double() - ref)[valid].abs().max())
    assert d < rs.TOL_LOGP, d
    decided = rs.argmax_decided(ref, valid)
    assert torch.equal(lp.argmax(-1)[decided], ref.argmax(-1)[decided])
    assert int(decided.sum()) >= (1 - rs.MAX_LEFT_OUT) * int(valid.sum()) - 1
    return d


def loss_tables(dev=DEV):
    from na_mpnn_amd import train
    rm, rn = train.polymer_restype_tables(RTI, 33, dev)
    no_loss = torch.tensor([RTI[t] for t in cpu_ref.NO_LOSS_TOKENS], device=dev)
    return rm, rn, no_loss


def flat_params(m):
    return torch.cat([p.detach().flatten() for p in m.parameters()]).clone()


def assert_within_spread(a, solos, what):
    """The rule of test_train_step_with_metrics_is_unchanged — identical solo runs differ through fp32 atomics by `spread`; the run under
    test must equal them when the spread is 0, else differ from each by at most 10 x spread — with the spread estimated from FOUR OR MORE
    identical solo runs (the largest pairwise difference): where atomics are in play the runs fall into a few discrete outcomes, two of
    which often coincide, so a two-run spread of 0 does not show reproducibility ("Call histories").  Equality is demanded
    only where all the solo runs coincide.  Prints and returns the spread."""
    assert len(solos) >= 4
    spread = max(float((x - y).abs().max()) for i, x in enumerate(solos) for y in solos[i + 1:])
    d = max(float((a - x).abs().max()) for x in solos)
    distinct = len({x.cpu().numpy().tobytes() for x in solos})
    print(f"{what}: {len(solos)} identical solo runs, {distinct} distinct outcomes, parameter spread {spread:.3e}; "
          f"largest difference of the run under test from a solo run {d:.3e}")
    if spread == 0.0:
        assert all(torch.equal(a, x) for x in solos), (what, d)
    else:
        assert d <= 10 * spread, (what, d, spread)
    return spread
