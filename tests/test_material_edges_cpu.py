"""The case list and the fp64 references of tests/material_edge_cases.py, checked without a GPU."""
import pytest
import torch

import material_edge_cases as mc


def test_every_class_of_the_work_split_has_a_case():
    assert mc.coverage_gaps() == []
    # the check is a condition on the list: it notices a class that loses its only case
    assert "tiles per round 3" in mc.coverage_gaps([n for n in mc.CASES if n != 32_769])
    assert "q 16 -> 32, both sides" in mc.coverage_gaps([n for n in mc.CASES if n != 16_384])
    assert "13 partials" in mc.coverage_gaps([n for n in mc.CASES if mc.REDUCE_CASES.get(n) != 13])
    assert "unsplit prologue" in mc.coverage_gaps([n for n in mc.CASES if mc.geometry(n)["split"]])


@pytest.mark.parametrize("n", sorted(mc.TABLE))
def test_geometry_equals_the_table(n):
    g = mc.geometry(n)
    assert (g["grid"], g["q"], g["tiles_per_round"], g["last_wave"], g["split"]) == mc.TABLE[n]
    assert g["last_tile"] == (g["last_wave"] - 1) % 16 + 1
    assert g["last_wg_waves_1_to_3_empty"] == (n - (g["grid"] - 1) * 4 * g["q"] <= g["q"])


def test_reduce_cases_give_the_wanted_number_of_partials():
    for n, k in mc.REDUCE_CASES.items():
        assert mc.wave_quota(n) == (k, 16)
        rows = mc.boundary_rows(n)
        assert all(64 * b in rows for b in range(k)) and rows == sorted(set(rows)) and 0 <= rows[0] and rows[-1] == n - 1
    for n in mc.CASES:
        grid, q = mc.wave_quota(n)
        want = {0, 15, 16, q - 1, q, 63, 64, 4 * q - 1, 4 * q, n - 17, n - 16, n - 2, n - 1}
        assert {r for r in want if 0 <= r < n} <= set(mc.boundary_rows(n))
        if n not in mc.REDUCE_CASES:
            assert len(mc.boundary_rows(n)) <= 13


def test_separated_inputs_stay_clear_of_the_adjoints_clamp():
    F = mc.separated_F()
    assert F.shape == (mc.N_MAX, 3, 3) and torch.equal(F, F.float().double())
    s = torch.linalg.svdvals(F.float()).double()          # what an fp32 SVD of the fp32 values sees
    assert float(s.min()) > 0.59 and float(s.max()) < 1.51
    gap = torch.minimum(s[:, 0] - s[:, 1], s[:, 1] - s[:, 2])
    assert float(gap.min()) > 0.099
    s2 = s * s
    assert float(torch.minimum(s2[:, 0] - s2[:, 1], s2[:, 1] - s2[:, 2]).min()) > 1e4 * mc.CLAMP
    assert float(torch.linalg.det(F).min()) > 0.0
    # ... and the further block is what the clamp is for: identities and tied singular values
    D = mc.degenerate_F(2 * mc.DEGENERATE_PERIOD + 3)
    sd = torch.linalg.svdvals(D)
    assert float(torch.minimum(sd[:, 0] - sd[:, 1], sd[:, 1] - sd[:, 2]).max()) < 1e-6
    assert torch.equal(D[:3], D[mc.DEGENERATE_PERIOD:mc.DEGENERATE_PERIOD + 3]) and torch.equal(D[0], torch.eye(3, dtype=torch.float64))


@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("n", [17, 65, 832])
def test_boundary_reference_is_the_sum_of_per_particle_gradients(kind, n):
    W = mc.weights("jelly", kind, lora=True)
    F, g = mc.separated_F()[:n], mc.boundary_gout(n)
    rows = mc.boundary_rows(n)
    assert sorted(set(torch.nonzero(g.abs().amax((1, 2)))[:, 0].tolist())) == rows
    gF, dW, noise = mc.boundary_ref(kind, n)
    assert 0.0 < noise["gF"] < 1e-3 and all(0.0 < v < 1e-3 for v in noise["dW"])      # the reference's own fp32 run: fp32-sized
    # one particle at a time
    acc = [torch.zeros_like(w) for w in W]
    for r in rows:
        _, gr, dr = mc.per_rows_ref(kind, F[r:r + 1], g[r:r + 1], W)
        assert float((gr[0] - gF[r]).abs().max()) <= 1e-13 * max(1.0, float(gF[r].abs().max()))
        acc = [a + d for a, d in zip(acc, dr)]
    for a, d in zip(acc, dW):
        assert float((a - d).abs().max()) <= 1e-13 * float(d.abs().max())
    # and the whole batch with the sparse cotangent: the rows without one add nothing
    _, gF_all, dW_all = mc.per_rows_ref(kind, F, g, W)
    assert float((gF_all - gF).abs().max()) <= 1e-13 * float(gF.abs().max())
    keep = torch.ones(n, dtype=torch.bool); keep[rows] = False
    assert float(gF_all[keep].abs().max()) == 0.0 if keep.any() else True
    for a, d in zip(dW_all, dW):
        assert float((a - d).abs().max()) <= 1e-13 * float(d.abs().max())


@pytest.mark.parametrize("kind", mc.KINDS)
def test_prefix_reference_equals_one_pass_in_any_order(kind):
    """PrefixRef adds the stretches between the counts asked for: same numbers as one fp64 pass over the first n rows, whatever
    the order of the requests"""
    ref = mc.PrefixRef(kind, mc.weights("jelly", kind, lora=True))
    for n in (257, 17, 320, 65):
        out, gF, dW, noise = ref.get(n)
        assert 0.0 < noise["gF"] < 1e-3 and all(0.0 < v < 1e-3 for v in noise["dW"])
        o1, g1, w1 = mc.per_rows_ref(kind, mc.separated_F()[:n], mc.dense_gout()[:n], ref.W)
        # (fp64 rounding only: the CPU's batched products are not bitwise independent of the batch they run in)
        assert out.shape == (n, 3, 3) and float((out - o1).abs().max()) <= 1e-13 * float(o1.abs().max())
        assert float((gF - g1).abs().max()) <= 1e-13 * float(g1.abs().max())
        for a, d in zip(dW, w1):
            assert float((a - d).abs().max()) <= 1e-12 * float(d.abs().max())
    fwd = mc.PrefixRef(kind, mc.weights("sand", kind, lora=False), with_grad=False)
    with torch.no_grad():
        whole = mc._apply(kind, mc.separated_F()[:300], fwd.W)
    assert float((fwd.get(300) - whole).abs().max()) <= 1e-13 * float(whole.abs().max()) and torch.equal(fwd.get(64), fwd.get(300)[:64])


def test_bound_is_the_suites_unless_the_references_own_fp32_run_is_further_off():
    assert mc.bound(1e-5, 2e-6) == 1e-5 and mc.bound(1e-5, 8e-6) == 1.6e-5 and mc.bound(2e-5, 0.0) == 2e-5
    assert mc.bound(1e-5, 1.0) == mc.bound(2e-5, 6e-5) == 2 * mc.NOISE_CAP == 1e-4          # capped


def _worst(noise):
    return max([noise["gF"]] + list(noise["dW"]))


@pytest.mark.parametrize("kind", mc.KINDS)
def test_the_references_own_fp32_run_stays_below_the_cap_at_every_count(kind):
    """the distance of the oracle's fp32 run from its fp64 run, which may widen a bound (material_edge_cases.bound), at every
    count of CASES and for both cotangents: below NOISE_CAP, so the cap of `bound` is idle and no bound is wider than
    2 x the figure printed here (seen: 2.0e-05 and 2.9e-05 on two hosts - the CPU's BLAS decides -, elasticity dL/dW1 under a
    boundary cotangent)"""
    worst = 0.0
    for n in mc.CASES:
        worst = max(worst, _worst(mc.dense_ref(kind, n)[3]), _worst(mc.boundary_ref(kind, n)[2]))
    print(f"[{kind}] largest fp32-vs-fp64 distance of the reference over CASES: {worst:.2e}")
    assert worst < mc.NOISE_CAP


def test_rollout_counts_have_the_geometry_they_are_there_for():
    for case, (n, _, _, want) in mc.ROLLOUT_EDGES.items():
        geo = mc.geometry(n)
        assert {k: geo[k] for k in want} == want, case
    assert mc.geometry(33)["last_wg_waves_1_to_3_empty"] is False and (33 - 1) // 16 == 2      # waves 0..2, wave 3 empty
