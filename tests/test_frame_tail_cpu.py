"""CPU: the inputs of test_gpu_frame_tail.py are what they claim to be - the exact data is exact (exactness condition, fp32
references), the structures hold the row lengths, empty rows and column patterns the kernels' edges need (a later edit of the
builder cannot drop one silently), the pixel shapes reach the launch paths they are listed for - and tune.Bindings builds the
CSR and the transposed CSR the kernels read."""
import numpy as np
import pytest
import torch

import frame_tail_cases as fc


# ---------------------------------------------------------------- structures
def _has_two_consecutive_empty(lengths):
    z = lengths == 0
    return bool((z[1:] & z[:-1]).any())


def test_lane_structures_hold_the_listed_rows():
    structs = fc.lane_structures()
    assert sorted(s.rows for s in structs if "samecol" not in s.name) == sorted(fc.LANE_ROWS) == [1, 15, 16, 17, 257]
    assert fc.LANE_LENGTHS == (0, 1, 15, 16, 17, 31, 32, 33, 48, 100)
    for s in structs:
        L = s.lengths
        if s.rows == 1:
            assert L[0] > 48                                     # several trips of sixteen lanes and a tail
            continue
        assert L[0] == 0 and L[-1] == 0 and _has_two_consecutive_empty(L), s.name
        assert set(fc.LANE_LENGTHS) <= set(L.tolist()), s.name


def test_bind_structures_hold_the_listed_rows():
    structs = fc.bind_structures()
    assert sorted(s.rows for s in structs if "samecol" not in s.name) == sorted(fc.BIND_K) == [1, 255, 256, 257]
    assert fc.BIND_LENGTHS == tuple(range(11)) + (16, 33)
    for s in structs:
        L = s.lengths
        if s.rows == 1:
            assert L[0] == 10                                    # the shipped maximum: two full trips and a tail of two
            continue
        assert L[0] == 0 and L[-1] == 0 and _has_two_consecutive_empty(L), s.name
        assert set(fc.BIND_LENGTHS) <= set(L.tolist()), s.name
        assert {int(x) % 4 for x in L if x > 0} == {0, 1, 2, 3}, s.name        # every tail residue of the four-per-trip loop


@pytest.mark.parametrize("structs", [fc.lane_structures, fc.bind_structures])
def test_column_patterns(structs):
    for s in structs():
        assert s.col.dtype == np.int32 and s.rowptr.dtype == np.int32 and s.val.dtype == np.float32
        for r in range(s.rows):                                  # rows ascend in column
            c = s.col[s.rowptr[r]:s.rowptr[r + 1]]
            assert (np.diff(c) >= 0).all(), (s.name, r)
        if "samecol" in s.name:
            assert len(set(s.col.tolist())) == 1
            continue
        assert 0 in s.col and s.ncols - 1 in s.col, s.name
        if s.rows > 1:
            assert s.repeated_rows().size == 1, s.name           # exactly one row repeats a column
    assert any("samecol" in s.name for s in structs())


def test_spmm_column_counts_cover_every_branch():
    assert fc.SPMM_D == (1, 2, 3, 4, 5, 9, 15, 16, 17, 33)


# ---------------------------------------------------------------- exactness
@pytest.mark.parametrize("s", fc.lane_structures() + fc.bind_structures(), ids=lambda s: s.name)
def test_exact_data_is_exact(s):
    rng = np.random.default_rng(1)
    assert fc.is_fp32(s.val.astype(np.float64) * 16) and (s.val >= 1 / 16).all() and (s.val <= 1).all()
    assert np.array_equal(s.val * 16, np.round(s.val * 16))
    assert fc.spmm_margin(s) < fc.EXACT_LIMIT
    for D in (3, 33):
        X = fc.exact_values(rng, (s.ncols, D))
        assert np.abs(X).max() <= 4 and np.array_equal(X * 16, np.round(X * 16))
        ref = fc.spmm_ref(s, X)
        assert np.array_equal(ref, ref.astype(np.float32))
        assert np.array_equal(ref * 256, np.round(ref * 256))                   # the granularity the margin assumes
    m_means, m_F = fc.bind_frame_margins(s)
    assert m_means < fc.EXACT_LIMIT and m_F < fc.EXACT_LIMIT
    pc, pp, kp = fc.exact_values(rng, (s.ncols, 3)), fc.exact_values(rng, (s.ncols, 3)), fc.exact_values(rng, (s.rows, 3))
    F = fc.exact_F(rng, (s.ncols, 9))
    assert np.abs(F).max() <= 4 and np.array_equal(F * 4, np.round(F * 4))
    means = kp.astype(np.float64) + fc.spmm_ref(s, pc.astype(np.float64) - pp.astype(np.float64))
    Fk = fc.spmm_ref(s, F)
    assert np.array_equal(means, means.astype(np.float32)) and np.array_equal(Fk, Fk.astype(np.float32))
    for n_in in (1, 4, 6):                                       # 6: the add-then-launch path of harness._tail_backward
        assert fc.sum3_margin(s, n_in) < fc.EXACT_LIMIT
        ins = [fc.exact_values(rng, (s.ncols, 3)).astype(np.float64) for _ in range(n_in)]
        for scale in (1.0, 0.25):
            ref = scale * fc.spmm_ref(s, sum(ins))
            assert np.array_equal(ref, ref.astype(np.float32))


def test_references_agree_with_dense_products():
    rng = np.random.default_rng(2)
    s = fc.by_name(fc.lane_structures(exact=False))["lane_r17"]
    X = fc.random_values(rng, (s.ncols, 5)); G = fc.random_values(rng, (s.rows, 3))
    np.testing.assert_allclose(fc.spmm_ref(s, X), s.dense() @ X.astype(np.float64), rtol=0, atol=1e-13)
    np.testing.assert_allclose(fc.spmm_t_ref(s, G), s.dense().T @ G.astype(np.float64), rtol=0, atol=1e-13)
    t = fc.transpose(s)
    assert np.array_equal(t.dense(), s.dense().T) and t.rows == s.ncols and t.ncols == s.rows
    b = fc.dot_bound(s, X, 1)
    assert b.shape == (s.rows, 5) and (b[s.lengths == 0] == 0).all() and (b[s.lengths > 0] > 0).all()
    cov6 = fc.random_values(rng, (4, 6)); F = fc.random_values(rng, (4, 9))
    ref, bound = fc.cov_push_ref(cov6, F)
    S = fc.sym6_to_33(cov6)
    assert np.array_equal(S, np.swapaxes(S, -1, -2)) and ref.shape == bound.shape == (4, 6) and (bound > 0).all()
    Fm = F.astype(np.float64).reshape(4, 3, 3)
    np.testing.assert_allclose(fc.sym6_to_33(ref), np.einsum("kab,kbc,kdc->kad", Fm, S, Fm), rtol=0, atol=1e-13)


# ---------------------------------------------------------------- pixel loss
@pytest.mark.parametrize("hw", list(fc.PIXEL_SHAPES), ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_pixel_shapes_reach_what_they_are_listed_for(hw):
    h, w = hw
    want = fc.PIXEL_SHAPES[hw]
    rule = fc.launch_rule(h, w)
    assert 3 * h * w < 65536
    assert rule["vec4"] == want["vec4"] and rule["grid"] == want["grid"]
    assert rule["row_trips"] == want.get("row_trips", 1) and rule["col_trips"] == want.get("col_trips", 1)
    assert not fc.launch_rule(h, w, aligned=False)["vec4"]
    weight, scale = fc.pow2_weight(h, w)
    assert 0.5 < weight <= 1.0 and np.float32(weight) == weight and np.log2(scale) == round(np.log2(scale))
    assert float(fc.fp32_scale(weight, h, w)) == scale           # the kernel's fp32 division gives the power of two
    assert fc.pixel_margin(h, w) < fc.EXACT_LIMIT
    for kind in (0, 1):
        a, g = fc.pixel_images(h, w, kind, exact=True)
        q = 256 if kind == 0 else 16
        assert np.array_equal(a * q, np.round(a * q)) and np.array_equal(g * q, np.round(g * q))
        assert a.min() >= 0 and a.max() <= 1 and g.min() >= 0 and g.max() <= 1
        assert (a == g).any() and (a > g).any() and (a < g).any()              # all three signs of the L1 gradient
        total = fc.pixel_term_sum(kind, a, g)
        assert total * 256 == round(total * 256)
        ref = fc.pixel_loss_ref(kind, weight, a, g)
        assert ref == total * scale and ref == float(np.float32(ref))
        stripes = [(0, h // 3), (h // 3, h // 3 + 1), (h // 3 + 1, h)]
        assert sum(fc.pixel_term_sum(kind, a, g, r0, r1) for r0, r1 in stripes if r1 > r0) == total
        grad = fc.pixel_grad_fp32(kind, scale, a, g)
        assert grad.dtype == np.float32
        exact = (np.sign(a.astype(np.float64) - g) if kind == 0 else 2.0 * (a.astype(np.float64) - g)) * scale
        assert np.array_equal(grad.astype(np.float64), exact)    # on exact data the fp32 expression is the exact gradient


def test_pixel_shapes_cover_every_launch_path():
    rules = [fc.launch_rule(h, w) for h, w in fc.PIXEL_SHAPES]
    for vec4 in (False, True):
        mine = [r for r in rules if r["vec4"] == vec4]
        assert any(r["grid"] == 512 for r in mine)               # the workgroup cap
        assert any(r["col_trips"] > 1 for r in mine)             # the inner loop's second trip
        assert any(r["row_trips"] > 1 for r in mine)             # the grid-strided second trip over rows
    assert any(r["grid"] == 128 and r["row_trips"] == 2 and r["vec4"] for r in rules)
    assert any(r["grid"] < 128 for r in rules)


# ---------------------------------------------------------------- tune.Bindings on the CPU
def _csr_dense(rowptr, col, val, shape):
    d = torch.zeros(shape, dtype=torch.float64)
    rows = torch.repeat_interleave(torch.arange(shape[0]), (rowptr[1:] - rowptr[:-1]).long())
    d.index_put_((rows, col.long()), val.double(), accumulate=True)
    return d


def _check_bindings(b, dense):
    K, N = dense.shape
    assert (b.K, b.N) == (K, N)
    for rowptr, col, val, nrows, ncols, want in ((b.rowptr, b.col, b.val, K, N, dense), (b.t_rowptr, b.t_col, b.t_val, N, K, dense.T)):
        assert rowptr.dtype == torch.int32 and col.dtype == torch.int32 and val.dtype == torch.float32
        assert rowptr.shape == (nrows + 1,) and int(rowptr[0]) == 0 and int(rowptr[-1]) == col.numel() == val.numel() == b.nnz
        assert bool((rowptr[1:] >= rowptr[:-1]).all())
        assert col.numel() == 0 or (int(col.min()) >= 0 and int(col.max()) < ncols)
        for r in range(nrows):
            c = col[int(rowptr[r]):int(rowptr[r + 1])]
            assert bool((c[1:] >= c[:-1]).all()), r              # rows ascend in column
        assert torch.equal(_csr_dense(rowptr, col, val, (nrows, ncols)), want.double())


def test_bindings_from_a_coalesced_sparse_tensor():
    from neuma_amd.tune import Bindings
    g = torch.Generator().manual_seed(0)
    K, N, nb = 37, 23, 5
    idx = torch.stack([torch.arange(K).repeat_interleave(nb), torch.randint(0, N, (K * nb,), generator=g)])
    val = torch.randint(1, 17, (K * nb,), generator=g).float() / 16          # dyadic: coalescing sums them exactly
    B = torch.sparse_coo_tensor(idx, val, (K, N)).coalesce()
    b = Bindings.from_sparse(B, device="cpu")
    assert b.nnz == B.values().numel() < K * nb                              # duplicates were merged by coalesce()
    _check_bindings(b, B.to_dense())
    counts = torch.bincount(B.indices()[0], minlength=K)
    assert torch.equal((b.rowptr[1:] - b.rowptr[:-1]).long(), counts)
    assert Bindings.of(b) is b


def test_bindings_from_raw_uncoalesced_indices():
    """duplicates of a (row, column) pair stay separate entries, next to each other, and both CSR copies sum to the dense matrix"""
    from neuma_amd.tune import Bindings
    s = fc.by_name(fc.lane_structures())["lane_r17"]
    perm = np.random.default_rng(3).permutation(s.col.size)                  # any order of the triples
    idx = torch.from_numpy(np.stack([s.row_of[perm], s.col.astype(np.int64)[perm]]))
    b = Bindings(idx, torch.from_numpy(s.val[perm]), (s.rows, s.ncols), device="cpu")
    assert b.nnz == s.col.size
    _check_bindings(b, torch.from_numpy(s.dense()))
    assert np.array_equal(b.rowptr.numpy(), s.rowptr) and np.array_equal(b.col.numpy(), s.col)
    rep = int(s.repeated_rows()[0])
    lo, hi = int(s.rowptr[rep]), int(s.rowptr[rep + 1])
    assert sorted(b.val[lo:hi].tolist()) == sorted(s.val[lo:hi].tolist())    # (the twins may swap places)
    keep = np.ones(s.col.size, dtype=bool); keep[lo:lo + 2] = False
    assert np.array_equal(b.val.numpy()[keep], s.val[keep])
    t = fc.transpose(s)
    assert np.array_equal(b.t_rowptr.numpy(), t.rowptr) and np.array_equal(b.t_col.numpy(), t.col)


def test_bindings_with_empty_rows_and_columns_and_all_empty():
    from neuma_amd.tune import Bindings
    dense = torch.zeros(6, 5)
    dense[1, 0], dense[1, 4], dense[4, 4], dense[3, 2] = 0.5, 0.25, 1.0, 0.75      # rows 0, 2, 5 and columns 1, 3 empty
    b = Bindings.from_sparse(dense.to_sparse(), device="cpu")
    _check_bindings(b, dense)
    assert b.rowptr.tolist() == [0, 0, 2, 2, 3, 4, 4] and b.col.tolist() == [0, 4, 2, 4] and b.val.tolist() == [0.5, 0.25, 0.75, 1.0]
    assert b.t_rowptr.tolist() == [0, 1, 1, 2, 2, 4] and b.t_col.tolist() == [1, 3, 1, 4] and b.t_val.tolist() == [0.5, 0.75, 0.25, 1.0]
    empty = Bindings.from_sparse(torch.zeros(4, 3).to_sparse(), device="cpu")
    _check_bindings(empty, torch.zeros(4, 3))
    assert empty.nnz == 0 and empty.rowptr.tolist() == [0] * 5 and empty.t_rowptr.tolist() == [0] * 4
