"""CPU tests of the specificity scan (ProteinMPNN.score_mutations with state_weights): the argument refusals and the
flat site / variant arrays, the size functions and the attach state machine of namp_state_mutations pinned without a device, and the
premises of the reference tests/state_scan_ref.py — the wild type has delta 0, equal states with weights summing to 1 are the single
state, and every GPU case tells a wrong combine from the right one.

Bars.  The wild type: the same fp64 rows on both sides, exactly 0.  Equal states: 1e-12 (fp64 throughout; measured below).  Sensitivity:
a mistaken reference (state_scan_ref.mistaken_fd) has to move some delta by 10 times the GPU tests' tolerance for that variant, 1e-3 x
its layer-3 rows.  Absent copies counted as present can be told only where a copy is absent (`unbound`, `LltK`), dropped weights only
where a weight is not 1 (every case but `single`): the other combinations leave nothing to get wrong, which is asserted too."""
import numpy as np
import pytest
import torch

from na_mpnn_amd import hip, spec
from na_mpnn_amd.model import MUT_MAX_EDITS, ProteinMPNN, _read_sections, _section_bytes, flat_sites_and_variants, output_section_layout
from oracle import cpu_ref
import context_states_ref as CR
import mutation_ref as MR
import state_scan_ref as SR

torch.set_grad_enabled(False)
EINVAL = -1
GPU_TOL = 1e-3                                               # per layer-3 row of the variant (tests/test_gpu_state_scan.py)


def host_model():
    return ProteinMPNN(num_letters=33, vocab=33, k_neighbors=16, atom_dict=spec.atom_dict(), restype_to_int=spec.restype_to_int(),
                       polytype_to_int=spec.polytype_to_int())


# ---- arguments ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    cx, fd, K, sites, tk = SR.case("LltK")
    m = host_model()
    M, L = fd["X"].shape[:2]
    for extra in (dict(symmetry_residues=[[0, 1]], symmetry_weights=[[1.0, 1.0]]), dict(paired_residues=[[0, 1]]),
                  dict(paired_wobble=True), dict(pair_terms={})):
        with pytest.raises(NotImplementedError, match="states alone"):
            m.score_mutations(dict(fd, **extra), sites=sites, site_tokens=tk)
    with pytest.raises(NotImplementedError, match="states alone"):
        m.score_mutations(fd, pairs=True)
    with pytest.raises(ValueError, match="mask \\* chain_mask == 0"):
        m.score_mutations(fd, positions=[25])                    # a fixed residue
    with pytest.raises(ValueError, match=f"3 residues in {M} states is 9 edits.*{MUT_MAX_EDITS}"):
        m.score_mutations(fd, sites=[[0, 1, 2]], site_tokens=[[0, 1, 2, 3]])
    with pytest.raises(ValueError):
        m.score_mutations(fd, method="sparse")
    with pytest.raises(ValueError):
        m.score_mutations(dict(fd, state_weights=[1.0, 2.0]), sites=sites, site_tokens=tk)      # M entries for M states
    with pytest.raises(RuntimeError):
        m.score_mutations(fd, sites=sites, site_tokens=tk)       # a CPU feature_dict, as for the other calls
    m4 = ProteinMPNN(num_letters=33, vocab=33, k_neighbors=16, num_decoder_layers=4, atom_dict=spec.atom_dict(),
                     restype_to_int=spec.restype_to_int(), polytype_to_int=spec.polytype_to_int())
    with pytest.raises(NotImplementedError, match="three decoder layers"):
        m4.score_mutations(fd, sites=sites, site_tokens=tk, method="cone")


def test_flat_sites_and_variants():
    """A site of s shared residues is s x M flat residues: every copy m * L + r, absent ones too, each with the residue's token."""
    cx, fd, K, sites, tk = SR.case("LltK")
    M, L = fd["X"].shape[:2]
    got = host_model()._state_scan_arguments(fd, None, None, sites, tk, False)
    state_w, M_, L_, ctx, st, tk_, scan, sites8, tok9 = got
    assert (M_, L_) == (M, L) and scan is None and np.array_equal(st, sites) and np.array_equal(tk_, tk)
    assert sites8.shape == (len(sites), 8) and tok9.shape == (len(tk), 9) and sites8.dtype == tok9.dtype == np.int32
    for q, row in enumerate(sites):
        assert sorted(sites8[q][sites8[q] >= 0].tolist()) == sorted(m * L + int(r) for r in row if r >= 0 for m in range(M))
    for v, row in enumerate(tk):
        q = int(row[0])
        assert tok9[v, 0] == q
        for e, f in enumerate(sites8[q]):
            if f >= 0:
                assert tok9[v, 1 + e] == row[1 + list(sites[q]).index(f % L)]
    # the scan form: the designable residues over their own alphabets, SHARED indices
    scan = host_model()._state_scan_arguments(fd, None, None, None, None, False)[6]
    cm = ((fd["mask"] * fd["chain_mask"])[0] != 0).nonzero()[:, 0].tolist()
    assert scan["positions"] == cm and scan["tokens"] == list(range(20))
    # two-residue sites in four states sit exactly at the cap
    cx, fd, K, sites, tk = SR.case("two_residue_sites")
    sites8 = host_model()._state_scan_arguments(fd, None, None, sites, tk, False)[7]
    assert (sites8 >= 0).all()


# ---- sizes and offsets ---------------------------------------------------------------------------------------------------------------
# (N, K, n_dec, n_states, n_sites, n_variants, list_1..3, items_1..3)
LEGAL = [(1, 1, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1), (34, 16, 3, 2, 2, 3, 4, 7, 9, 6, 10, 14),
         (96, 8, 3, 8, 2, 3, 16, 20, 24, 24, 30, 36), (1000, 48, 3, 4, 100, 2000, 300, 900, 2500, 6000, 18000, 50000),
         (34, 16, 3, 2, 2, 0, 0, 0, 0, 0, 0, 0)]
REFUSED = [(34, 16, 4, 2, 2, 3, 4, 7, 9, 6, 10, 14), (34, 36, 3, 2, 2, 3, 4, 7, 9, 6, 10, 14), (34, 16, 3, 2, 0, 3, 4, 7, 9, 6, 10, 14),
           (34, 16, 3, 2, 2, 3, 4, 7, 9, 6, 10, -1), (34, 16, 3, 2, 2, 3, 4, 7, 9, 6, 10, 1 << 28),
           # n_states: 0, negative, past NAMP_MUT_MAX_EDITS, no divisor of N
           (34, 16, 3, 0, 2, 3, 4, 7, 9, 6, 10, 14), (34, 16, 3, -2, 2, 3, 4, 7, 9, 6, 10, 14), (36, 16, 3, 9, 2, 3, 4, 7, 9, 6, 10, 14),
           (34, 16, 3, 4, 2, 3, 4, 7, 9, 6, 10, 14)]


def _sizes(dims):
    Lb = hip.lib()
    return tuple(int(getattr(Lb, "namp_state_mutations" + f)(*dims)) for f in ("_workspace_bytes", "_in_offset", "_out_offset"))


def _round(elems):
    return (4 * elems + 255) // 256 * 256


@pytest.mark.parametrize("dims", LEGAL)
def test_sections_are_aligned_ordered_and_hold_what_the_header_lists(dims):
    N, K, n_dec, M, ns, nv, l1, l2, l3, i1, i2, i3 = dims
    size, i_off, o_off = _sizes(dims)
    plain = tuple(int(getattr(hip.lib(), "namp_mutations" + f)(*(dims[:3] + dims[4:])))
                  for f in ("_workspace_bytes", "_in_offset", "_out_offset"))
    assert 0 < i_off < o_off < size and i_off % 256 == o_off % 256 == size % 256 == 0
    assert i_off == plain[1]                                      # the scan's own buffers come first, unchanged
    # the output section: sizes, delta, state_delta, rows (2), units (2), base units — each with ONE extra element, rounded to 256
    out = sum(_round(e + 1) for e in (3 * ns, nv, nv * M, i3, i3, i3, i3, N // M))
    assert size - o_off == out
    # what the specificity scan adds to the plain scan: unit_w [N] in the input section, the whole rows and the terms, four output arrays
    add_in = _round(ns * 8 + nv * 9 + 2 * N) - _round(ns * 8 + nv * 9 + N)
    add = add_in + _round(i3 * 64 + 4) + _round(i3 + 1) + _round(nv * M + 1) + 2 * _round(i3 + 1) + _round(N // M + 1)
    assert size == plain[0] + add


def _section_total(family, dims):
    return sum(_section_bytes(elems) for _, elems, _ in output_section_layout(family, dims))


@pytest.mark.parametrize("dims", LEGAL)
def test_the_python_layout_is_the_output_section_of_both_scans(dims):
    """output_section_layout against the library's own sizes, and against the arrays include/namp.h lists, in its order."""
    N, K, n_dec, M, ns, nv, l1, l2, l3, i1, i2, i3 = dims
    i32, f32 = torch.int32, torch.float32
    size, _, o_off = _sizes(dims)
    assert _section_total("state_mutations", dims) == size - o_off
    assert [(e, t) for _, e, t in output_section_layout("state_mutations", dims)] == [
        (3 * ns, i32), (nv, f32), (nv * M, f32), (i3, i32), (i3, f32), (i3, i32), (i3, f32), (N // M, f32)]
    plain = dims[:3] + dims[4:]
    Lb = hip.lib()
    assert _section_total("mutations", plain) == int(Lb.namp_mutations_workspace_bytes(*plain)) - int(Lb.namp_mutations_out_offset(*plain))
    assert [(e, t) for _, e, t in output_section_layout("mutations", plain)] == [(3 * ns, i32), (nv, f32), (i3, i32), (i3, f32)]
    # the reader walks the same bytes: every view starts 256-aligned, holds its elems, and the last one ends inside the section
    ws = torch.zeros(size - o_off + 256, dtype=torch.uint8)
    views = _read_sections(ws, 256, output_section_layout("state_mutations", dims))
    assert list(views) == ["site_rows", "delta", "state_delta", "row_residue", "row_token_log_prob", "unit_residue", "unit_log_prob",
                           "base_units"]
    for (name, elems, dtype), v in zip(output_section_layout("state_mutations", dims), views.values()):
        assert v.dtype == dtype and v.numel() == elems and 4 * v.storage_offset() % 256 == 0
    last = views["base_units"]
    assert 4 * last.storage_offset() + _section_bytes(last.numel()) == ws.numel()


# small and large shapes of tests/test_workspace_layout_host.py: (N, K, n_dec, n_var, n_chunk, rows_1..3) / (N, K, n_dec, n_tables, n_classes, n_chunk)
@pytest.mark.parametrize("family,dims,want", [
    ("library", (1, 1, 3, 1, 1, 1, 1, 1), [(63, torch.int32), (1, torch.float32)]),
    ("library", (1000, 48, 3, 40, 64, 60, 150, 400), [(63, torch.int32), (64000, torch.float32)]),
    ("tied_score", (1, 1, 3, 1, 33, 1), [(63, torch.int32), (1, torch.float32), (1, torch.float32)]),
    ("tied_score", (1000, 48, 3, 64, 64, 65), [(63, torch.int32), (65000, torch.float32), (65000, torch.float32)])])
def test_the_python_layout_of_the_library_and_the_tied_score(family, dims, want):
    """A 64-word header (carved as it stands: 63 + 1), then float [n_chunk][N] once / twice, as include/namp.h lists them."""
    Lb = hip.lib()
    size, o_off = (int(getattr(Lb, f"namp_{family}{f}")(*dims)) for f in ("_workspace_bytes", "_out_offset"))
    assert 0 < o_off < size and _section_total(family, dims) == size - o_off
    assert [(e, t) for _, e, t in output_section_layout(family, dims)] == want
    assert _section_bytes(63) == 256


def _flat_by_loops(st, tk, M, L):
    """The arrays of flat_sites_and_variants spelled out: per site, per listed residue, per state."""
    sites8 = np.full((len(st), MUT_MAX_EDITS), -1, np.int32)
    tok9 = np.zeros((len(tk), 1 + MUT_MAX_EDITS), np.int32)
    tok9[:, 0] = tk[:, 0]
    for q, row in enumerate(st):
        cols = [c for c, r in enumerate(row) if r >= 0]
        pick = np.nonzero(tk[:, 0] == q)[0]
        for e, c in enumerate(cols):
            for m_ in range(M):
                sites8[q, e * M + m_] = m_ * L + row[c]
                tok9[pick, 1 + e * M + m_] = tk[pick, 1 + c]
    return sites8, tok9


@pytest.mark.parametrize("name,st,tk,M,L", [
    ("M=1", [[3, 5, 7], [9, 11, 2]], [[1, 4, 5, 6], [0, 1, 2, 3], [1, 7, 8, 9], [0, 20, 21, 22]], 1, 12),
    ("M=1, eight residues", [list(range(8, 0, -1))], [[0] + list(range(10, 18))], 1, 9),
    ("M=4 at the cap", [[3, 5], [0, 11]], [[1, 4, 5], [0, 1, 2], [1, 7, 8]], 4, 12),
    ("a padded site row", [[3, -1], [4, 6], [8, -1]], [[2, 9, 0], [0, 1, 0], [1, 2, 3], [0, 5, 0]], 3, 10),
    ("a padded row of three columns in four states", [[3, -1, -1], [4, 6, -1]], [[1, 2, 3, 0], [0, 1, 0, 0]], 4, 10),
    ("n=0", [[3, 5], [0, 11]], np.zeros((0, 3), np.int64), 4, 12),
    ("no site", np.zeros((0, 1), np.int64), np.zeros((0, 2), np.int64), 2, 12)])
def test_the_padding_of_sites_and_variants_against_loops(name, st, tk, M, L):
    st, tk = np.asarray(st, np.int64), np.asarray(tk, np.int64)
    sites8, tok9 = flat_sites_and_variants(st, tk, M, L)
    want8, want9 = _flat_by_loops(st, tk, M, L)
    assert sites8.dtype == tok9.dtype == np.int32 and sites8.shape == (len(st), 8) and tok9.shape == (len(tk), 9)
    assert np.array_equal(sites8, want8) and np.array_equal(tok9, want9)
    if M == 1 and (st >= 0).all():                                # the plain scan: the arrays as they are, padded
        assert np.array_equal(sites8[:, :st.shape[1]], st) and np.array_equal(tok9[:, :tk.shape[1]], tk)
    if name == "M=4 at the cap":
        assert (sites8 >= 0).all() and sites8[0].tolist() == [3, 15, 27, 39, 5, 17, 29, 41] and tok9[0].tolist() == [1, 4, 4, 4, 4, 5, 5, 5, 5]


@pytest.mark.parametrize("dims", REFUSED)
def test_refused_dims_give_zero(dims):
    assert _sizes(dims) == (0, 0, 0)


# ---- the state machine, without a device: every carrier call below fails before any launch -----------------------------------------
def _carried(N=10, K=4):
    Lb = hip.lib()
    assert Lb.namp_decoder_fwd(None, None, None, None, None, None, None, None, None, None, None, 0, 1, 1, N, K, None) == EINVAL
    return Lb.namp_last_error()


def test_state_machine_without_a_device():
    Lb = hip.lib()
    attach = lambda: Lb.namp_state_mutations(2, 5, 1, 0, 0, 0, 0, 0, 0, 0)
    plain = lambda msg: b"null weights" in msg and b"attached" not in msg
    assert plain(_carried())
    assert attach() == 0
    msg = _carried()
    assert b"a state scan was attached" in msg and b"null pointer" in msg
    assert plain(_carried())                                      # taken and cleared by the call that failed
    assert attach() == 0 and attach() == 0                        # the same kind again replaces it: no conflict
    assert b"a state scan was attached" in _carried() and plain(_carried())
    for bad in ((0, 5, 1, 0, 0, 0, 0, 0, 0, 0), (9, 5, 1, 0, 0, 0, 0, 0, 0, 0), (2, 0, 1, 0, 0, 0, 0, 0, 0, 0), (2, 5, 1, 0, 0, 0, 0, 0, 0, -1),
                (2, 5, -1, 0, 0, 0, 0, 0, 0, 0)):
        assert attach() == 0 and Lb.namp_state_mutations(*bad) == EINVAL  # a refused attach of the same kind leaves it cleared
        assert b"namp_state_mutations" in Lb.namp_last_error()
        assert plain(_carried())
    others = {b"library": lambda: Lb.namp_library(1, 0, 0, 0, 0), b"mutational scan": lambda: Lb.namp_mutations(1, 0, 0, 0, 0, 0, 0, 0),
              b"tied score": lambda: Lb.namp_tied_score(1, 33, 2)}
    for noun, other in others.items():
        for first, second in ((attach, other), (other, attach)):
            assert first() == 0 and second() == 0                 # two kinds: neither runs, both named, both gone
            msg = _carried()
            assert noun in msg and b"state scan" in msg and b"were attached together" in msg and b"null" not in msg
            assert plain(_carried())
    assert attach() == 0 and Lb.namp_mutations(1, 0, 0, 0, 0, 0, 0, -1) == EINVAL      # a refused attach of another kind leaves this one
    assert b"a state scan was attached" in _carried() and plain(_carried())
    assert attach() == 0 and all(f() == 0 for f in others.values())  # all four at once
    msg = _carried()
    assert all(noun in msg for noun in others) and b"state scan" in msg and plain(_carried())


def test_the_record_belongs_to_the_calling_thread():
    import threading
    Lb = hip.lib()
    assert Lb.namp_state_mutations(2, 5, 1, 0, 0, 0, 0, 0, 0, 0) == 0
    seen = []
    t = threading.Thread(target=lambda: seen.append(_carried()))
    t.start()
    t.join()
    assert b"attached" not in seen[0]                            # another thread's call carries nothing
    assert b"a state scan was attached" in _carried()            # ... and this thread's record is still there


# ---- the reference -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs():
    """The reference of every GPU case, computed once and left unchanged."""
    out = {}
    for name in SR.CASES:
        cx, fd, K, sites, tk = SR.case(name)
        out[name] = SR.reference(fd, K, sites, tk)
    return out


@pytest.mark.parametrize("name", SR.CASES)
def test_the_wild_type_has_delta_zero(refs, name):
    cx, fd, K, sites, tk = SR.case(name)
    ref = refs[name]
    S = cx["S"]
    wild = [v for v, row in enumerate(tk) if all(int(S[r]) == int(t) for r, t in zip(sites[row[0]], row[1:]) if r >= 0)]
    assert len(wild) >= 2
    assert float(ref["delta"][wild].abs().max()) == 0 and float(ref["state_delta"][wild].abs().max()) == 0
    assert float(ref["delta"].abs().max()) > 0.1                  # ... and the mutants are felt
    M, L = fd["X"].shape[:2]
    assert ref["delta"].dtype == torch.float64 and ref["state_delta"].shape == (len(tk), M) and ref["units"].shape == (len(tk) + 1, L)


def test_equal_states_with_weights_summing_to_one_are_the_single_state():
    """Two copies of one backbone under the weights (0.6, 0.4), everything in fp64: the unit is log_softmax(0.6 lp + 0.4 lp) = lp, so
    the scan is the single-state scan — the delta of tests/mutation_ref's explicit sequences under score() — within 1e-12."""
    cx, fd, K, sites, tk = SR.case("plain")
    w64 = cpu_ref.to_dtype(SR.weights_t(), torch.float64)
    fd2 = cpu_ref.to_dtype(dict(fd, X=fd["X"][:1].repeat(2, 1, 1, 1), state_weights=[0.6, 0.4]), torch.float64)
    S_all = SR.sequences(fd2, sites, tk)
    got = CR.oracle_score_tied(w64, fd2, K, S_all)
    delta = got["log_likelihood"][:-1] - got["log_likelihood"][-1]
    one = cpu_ref.to_dtype({k: v for k, v in CR.context_state_fd(fd2, 0).items() if k != "state_weights"}, torch.float64)
    h_V, h_E, E_idx = cpu_ref.encode(w64, one, K)
    cm = (one["mask"] * one["chain_mask"])[0]
    own = []
    for S_k in torch.from_numpy(MR.expand(cx["S"], sites, tk)).long().tolist() + [cx["S"].tolist()]:
        S_k = torch.tensor(S_k)
        lp = cpu_ref.score_from_encoded(w64, h_V, h_E, E_idx, S_k[None], one["mask"], one["chain_mask"], one["randn"][:1], 1)["log_probs"]
        assert lp.dtype == torch.float64
        own.append(torch.log_softmax(lp[0], -1).gather(1, S_k[:, None])[:, 0])
    own = torch.stack(own)
    single = ((own[:-1] - own[-1:]) * cm[None]).sum(-1)
    d = float((delta - single).abs().max())
    print(f"equal states vs the single state: max |d delta| = {d:.3e} (|delta| up to {float(single.abs().max()):.2f})")
    assert float(single.abs().max()) > 0.1 and d < 1e-12
    sd = got["state_log_likelihood"][:-1] - got["state_log_likelihood"][-1:]
    assert float((sd - single[:, None]).abs().max()) < 1e-12     # every state's own figure is the single state's too


@pytest.mark.parametrize("name,mistake", [(n, "absent_as_present") for n in ("unbound", "LltK")] +
                         [(n, "drop_weights") for n in SR.CASES if n != "single"])
def test_the_cases_tell_a_mistaken_reference_from_the_right_one(refs, name, mistake):
    """Measured: absent copies as present — unbound 214, LltK 93 times the tolerance; the weights dropped — tokens_deformed 1129, unbound
    1054, LltK 2641, plain 837, cap8 2915, two_residue_sites 354 times."""
    cx, fd, K, sites, tk = SR.case(name)
    rows = SR.flat_rows(fd, K, sites)[0][tk[:, 0], 2]
    wrong = SR.reference(SR.mistaken_fd(fd, mistake), K, sites, tk)["delta"]
    moved = (wrong - refs[name]["delta"]).abs().numpy() / (GPU_TOL * rows)
    print(f"{name} {mistake}: a delta moves by {moved.max():.1f} x its GPU tolerance (rows {rows.tolist()})")
    assert moved.max() >= 10.0


def test_the_other_combinations_leave_nothing_to_get_wrong():
    """No copy is absent outside `unbound` and `LltK`; the one weight of `single` is 1."""
    for name in SR.CASES:
        fd = SR.case(name)[1]
        assert (SR.mistaken_fd(fd, "absent_as_present") is None) == (name not in ("unbound", "LltK"))
        assert (SR.mistaken_fd(fd, "drop_weights") is None) == (name == "single")
