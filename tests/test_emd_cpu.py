"""CPU: the numpy twin of the earth mover's distance (neuma_amd/extras/emd.py) against scipy's exact assignment solver on every
case of tests/emd_cases.py, its certificate, its repeatability, the round-count table behind the default round limit, and the
host side of `python -m neuma_amd.particle_evaluation --emd` (flags, subsampling, the _emd.txt writer)."""
import functools
import math

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import emd_cases as K
from gpu_util import measured

CASE_POWER = [(name, p) for name in K.CASES for p in K.POWERS]


def _E():
    from neuma_amd.extras import emd
    return emd


@functools.lru_cache(maxsize=None)
def scipy_optimum(name, power):
    C = K.twin(name, power)["C"]
    r, c = linear_sum_assignment(C)
    return int(C[r, c].sum())


@pytest.mark.parametrize("name,power", CASE_POWER)
def test_twin_is_an_exact_optimum_of_the_quantised_problem(name, power):
    E = _E()
    t = K.twin(name, power)
    n, C = K.CASES[name][1], t["C"]
    assert C.dtype == np.int64 and int(C.min()) >= 0 and int(C.max()) <= 2 ** 24
    assert sorted(t["idx"].tolist()) == list(range(n)), "idx is not a permutation"
    mine = int(C[np.arange(n), t["idx"]].sum())
    print(f"{name} p={power}: rounds {t['rounds']} ({t['rounds'] / n:.2f} n), sum C {mine}, scipy {scipy_optimum(name, power)}")
    assert measured(abs(mine - scipy_optimum(name, power)), "sum C - scipy optimum") <= 0         # integer equality
    # 1-complementary slackness on Cs = C (n + 1): the certificate the guarantee is derived from
    assert measured(E.slackness_violation(C, t["idx"], t["prices"]), "slackness violation") <= 1
    assert int(t["prices"].min()) >= 0 and int(t["prices"].max()) < 2 ** 50


@pytest.mark.parametrize("name,power", [(n, p) for n, p in CASE_POWER if K.CASES[n][1] <= 512])
def test_twin_twice_gives_identical_results(name, power):
    a, b = K.case(name)
    t, u = K.twin(name, power), _E().solve(a, b, power)
    assert np.array_equal(t["idx"], u["idx"]) and np.array_equal(t["prices"], u["prices"]) and t["rounds"] == u["rounds"]
    assert t["emd"] == u["emd"] or (math.isnan(t["emd"]) and math.isnan(u["emd"]))


@pytest.mark.parametrize("name", ["uniform2", "uniform65", "permuted_jitter256", "collinear256", "offset256"])
@pytest.mark.parametrize("power", K.POWERS)
def test_value_is_within_one_quantum_of_the_fp64_optimum(name, power):
    """the reported value exceeds the true fp64 optimum by at most 2^-k <= Cmax 2^-23 (and is no smaller than it, up to the
    rounding of two fp64 sums of n terms)"""
    E = _E()
    a, b = K.case(name)
    t = K.twin(name, power)
    c = E.costs(a, b, power)
    r, cc = linear_sum_assignment(c)
    best = math.fsum(c[r, cc]) / len(a)
    cmax, k = E.cost_scale(a, b, power)
    assert 2.0 ** -k <= cmax * 2.0 ** -23
    assert measured(t["emd"] - best, "emd - fp64 optimum") <= 2.0 ** -k
    assert measured(best - t["emd"], "fp64 optimum - emd") <= 4 * np.finfo(np.float64).eps * best


def test_degenerate_and_special_cases():
    E = _E()
    t = K.twin("identical100", 1)
    assert t["emd"] == 0.0 and t["rounds"] == 0 and np.array_equal(t["idx"], np.arange(100)) and not t["prices"].any()
    for p in K.POWERS:
        assert K.twin("exact_permutation512", p)["emd"] == 0.0          # exactly 0, not merely small
        a, b = K.case("exact_permutation512")
        assert np.array_equal(a, b[K.twin("exact_permutation512", p)["idx"]])
    a, b = K.case("uniform1")
    d = a.astype(np.float64) - b.astype(np.float64)
    assert K.twin("uniform1", 2)["emd"] == float((d[0, 0] * d[0, 0] + d[0, 1] * d[0, 1]) + d[0, 2] * d[0, 2])
    bad = np.array(K.case("uniform64")[0])
    bad[5, 1] = np.nan
    r = E.solve(bad, K.case("uniform64")[1], 1)
    assert math.isnan(r["emd"]) and (r["idx"] == -1).all() and r["rounds"] == 0
    with pytest.raises(RuntimeError, match="round limit"):
        E.solve(*K.case("clusters1024"), 1, max_rounds=4)


def test_cpu_path_takes_tensors_arrays_and_batches():
    E = _E()
    a, b = K.case("uniform63")
    t = K.twin("uniform63", 1)
    v, idx = E.earth_movers_distance(torch.from_numpy(np.array(a)), torch.from_numpy(np.array(b)), 1, give_id=True)
    assert v == t["emd"] and np.array_equal(idx, t["idx"])
    assert E.earth_movers_distance(a.astype(np.float64), b.astype(np.float64), 1) == t["emd"]
    vb = E.earth_movers_distance(np.stack([a, b]), np.stack([b, a]), 2)
    assert vb.shape == (2,) and vb[0] == K.twin("uniform63", 2)["emd"]
    assert measured(abs(vb[0] - vb[1]), "EMD(a, b) - EMD(b, a)") <= 2.0 ** -E.cost_scale(a, b, 2)[1]      # symmetric up to one quantum
    with pytest.raises(ValueError, match="subsample"):
        E.earth_movers_distance(a, b[:60], 1)
    with pytest.raises(ValueError, match="power"):
        E.earth_movers_distance(a, b, 3)
    with pytest.raises(ValueError, match="8192"):
        E.quantised_costs(np.zeros((8193, 3), np.float32), np.zeros((8193, 3), np.float32), 1)


def test_round_count_table_behind_the_default_round_limit():
    """default max_rounds = 16 x the largest rounds / n of the twin over the cases x powers, times n"""
    E = _E()
    table = {(name, p): K.twin(name, p)["rounds"] / K.CASES[name][1] for name, p in CASE_POWER}
    worst = max(table, key=table.get)
    print("rounds / n:", {f"{k[0]}/p{k[1]}": round(v, 2) for k, v in table.items()})
    assert worst == ("collinear256", 1)
    assert table[worst] == E.ROUNDS_PER_POINT_SEEN == 26672 / 256
    assert E.ROUNDS_MARGIN == 16 and E.MAX_ROUNDS_PER_POINT == math.ceil(E.ROUNDS_MARGIN * E.ROUNDS_PER_POINT_SEEN) == 1667
    assert E.default_max_rounds(4096) == 1667 * 4096


def test_subsample_indices_sorted_unique_seeded():
    from neuma_amd.particle_metrics import subsample_indices
    s = subsample_indices(5000, 128, 0)
    assert s.dtype == np.int64 and s.shape == (128,) and (np.diff(s) > 0).all() and s[0] >= 0 and s[-1] < 5000
    assert np.array_equal(s, subsample_indices(5000, 128, 0))
    assert not np.array_equal(s, subsample_indices(5000, 128, 1))
    assert np.array_equal(s, np.sort(np.random.default_rng(0).permutation(5000)[:128]))
    assert np.array_equal(subsample_indices(100, 100, 3), np.arange(100))
    assert np.array_equal(subsample_indices(100, 4096, 3), np.arange(100))


def test_entry_point_flags_and_emd_file(tmp_path):
    from neuma_amd import particle_evaluation as pe
    a = pe.parse_args(["-p", "x/states_run", "-g", "y"])
    assert (a.emd, a.emd_points, a.emd_power, a.emd_seed) == (False, 4096, 1, 0)
    a = pe.parse_args(["-p", "x", "-g", "y", "--emd", "--emd_points", "128", "--emd_power", "2", "--emd_seed", "7"])
    assert (a.emd, a.emd_points, a.emd_power, a.emd_seed) == (True, 128, 2, 7)
    with pytest.raises(SystemExit):
        pe.parse_args(["-p", "x", "-g", "y", "--emd_power", "3"])
    assert pe.emd_points_used(3000, 2500, 4096) == 2500 and pe.emd_points_used(3000, 2500, 128) == 128
    assert pe.emd_points_used(20000, 30000, 100000) == 8192
    run = tmp_path / "states_run"
    run.mkdir()
    assert pe.emd_path(str(run)).endswith("states_run/../states_run_emd.txt")
    pe.write_emd(pe.emd_path(str(run)), [0, 2], [1.5e-2, 2.5e-2], [128, 128], [700, 12])
    assert (tmp_path / "states_run_emd.txt").read_text() == ("frame EMD n rounds\n000 1.50000000e-02 128 700\n"
                                                             "002 2.50000000e-02 128 12\nmean 2.00000000e-02\n")
