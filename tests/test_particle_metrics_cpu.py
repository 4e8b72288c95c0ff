"""CPU: the host side of `python -m neuma_amd.particle_evaluation` - flags, frame names, the missing-file error, the grouping of
frames into nm_chamfer batches, the metrics file - and the internal consistency of the Chamfer fixtures
(tests/golden/chamfer/*.npz, made by the reference's metrics.py) against an fp64 numpy brute force.  None of this opens
libneuma_hip.so."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLD))
import chamfer_inputs as CI  # noqa: E402


def test_flags_and_defaults():
    from neuma_amd.particle_evaluation import parse_args
    a = parse_args([])
    assert (a.pred_dir, a.gt_dir, a.start, a.skip, a.num, a.device) == (None, None, 0, 1, 10, "cuda")
    a = parse_args(["-p", "P", "-g", "G", "-s", "3", "-k", "2", "-n", "4", "-d", "cuda:1"])
    assert (a.pred_dir, a.gt_dir, a.start, a.skip, a.num, a.device) == ("P", "G", 3, 2, 4, "cuda:1")
    a = parse_args(["--pred_dir", "P", "--gt_dir", "G", "--start", "1", "--skip", "5", "--num", "2", "--device", "cuda"])
    assert (a.pred_dir, a.gt_dir, a.start, a.skip, a.num) == ("P", "G", 1, 5, 2)


def test_frame_indices_follow_the_image_evaluation():
    from neuma_amd import evaluation
    from neuma_amd.particle_evaluation import frame_indices
    for args in ((0, 1, 10), (3, 2, 4), (5, 3, 0)):
        assert frame_indices(*args) == evaluation.frame_indices(*args)
    assert frame_indices(3, 2, 4) == [3, 5, 7, 9, 11]


def test_frame_names_and_the_missing_file_error(tmp_path):
    from neuma_amd.particle_evaluation import frame_paths
    pred, gt = tmp_path / "pred", tmp_path / "gt"
    pred.mkdir()
    gt.mkdir()
    with pytest.raises(FileNotFoundError, match=str(pred / "007.ply")):      # the prediction is checked first
        frame_paths(str(pred), str(gt), 7)
    (pred / "007.ply").write_bytes(b"")
    with pytest.raises(FileNotFoundError, match=str(gt / "007.ply")):
        frame_paths(str(pred), str(gt), 7)
    (gt / "007.ply").write_bytes(b"")
    assert frame_paths(str(pred), str(gt), 7) == (str(pred / "007.ply"), str(gt / "007.ply"))


def test_grouping_of_frames_into_batches():
    from neuma_amd.particle_evaluation import CHUNK, group_frames
    assert CHUNK == 64
    assert group_frames([]) == []
    assert group_frames([(5, 6)]) == [[0]]
    s = [(5, 6), (5, 6), (5, 7), (5, 6), (5, 6), (5, 6)]
    assert group_frames(s) == [[0, 1], [2], [3, 4, 5]]                       # only CONSECUTIVE equal sizes share a batch
    assert group_frames(s, chunk=2) == [[0, 1], [2], [3, 4], [5]]
    g = group_frames([(3, 3)] * 130)
    assert [len(x) for x in g] == [64, 64, 2] and sum(g, []) == list(range(130))


def test_metrics_file_layout(tmp_path):
    from neuma_amd.particle_evaluation import metrics_path, write_metrics
    pred = tmp_path / "states_run"
    pred.mkdir()
    path = metrics_path(str(pred))
    assert Path(path).resolve() == tmp_path / "states_run_chamfer.txt"
    assert Path(metrics_path(str(pred) + "/")).resolve() == tmp_path / "states_run_chamfer.txt"
    c12, c21 = [1.0, 2.5, 0.25], [0.5, 0.5, 4.0]
    write_metrics(path, [0, 2, 4], [a + b for a, b in zip(c12, c21)], c12, c21)
    lines = Path(path).read_text().splitlines()
    assert lines[0].split() == ["frame", "CD", "pred_to_gt", "gt_to_pred"]
    rows = [ln.split() for ln in lines[1:]]
    assert [r[0] for r in rows] == ["000", "002", "004", "mean"]
    vals = np.array([[float(v) for v in r[1:]] for r in rows])
    np.testing.assert_allclose(vals[:3, 1], c12, rtol=1e-8)
    np.testing.assert_allclose(vals[:3, 2], c21, rtol=1e-8)
    np.testing.assert_allclose(vals[:3, 0], vals[:3, 1] + vals[:3, 2], rtol=1e-8)
    np.testing.assert_allclose(vals[3], vals[:3].mean(0), rtol=1e-8)


def _brute(q, t):
    """fp64 squared distances of every query to every target: (N, M)"""
    q, t = q.astype(np.float64), t.astype(np.float64)
    return ((q[:, None, :] - t[None, :, :]) ** 2).sum(-1)


@pytest.mark.parametrize("name", sorted(CI.KDTREE_CASES))
def test_kdtree_fixtures_agree_with_an_fp64_brute_force(name):
    p1, p2 = CI.KDTREE_CASES[name]()
    g = np.load(GOLD / "chamfer" / f"{name}.npz")
    B, N, M = p1.shape[0], p1.shape[1], p2.shape[1]
    assert g["idx12"].shape == (B, N) and g["idx21"].shape == (B, M) and g["idx12"].dtype == np.int32
    for b in range(B):
        d = _brute(p1[b], p2[b])
        for dd, idx, c in ((d, g["idx12"][b], g["chamfer1"][b]), (d.T, g["idx21"][b], g["chamfer2"][b])):
            best = dd.min(1)
            assert np.array_equal(dd[np.arange(len(idx)), idx], best)            # every fixture index is a nearest neighbour
            assert abs(float(c) - best.mean()) <= 2e-6 * best.mean()               # the reference's fp32 mean
    np.testing.assert_allclose(g["chamfer"], g["chamfer1"] + g["chamfer2"], rtol=1e-6)
    if name == "duplicates":                                                      # ties are present where they should be
        d = _brute(p1[0], p2[0])
        assert ((d == d.min(1, keepdims=True)).sum(1) == 4).all()


def test_naive_fixture_agrees_with_an_fp64_brute_force():
    p1, p2 = CI.naive()
    g = np.load(GOLD / "chamfer" / "naive.npz")
    for b in range(p1.shape[0]):
        d = _brute(p1[b], p2[b])
        ref = d.min(1).mean() + d.min(0).mean()
        assert abs(float(g["chamfer"][b]) - ref) <= 2e-6 * ref


def test_fixture_inputs_are_deterministic_and_small():
    total = 0
    for make in list(CI.KDTREE_CASES.values()) + list(CI.NAIVE_CASES.values()):
        a1, b1 = make()
        a2, b2 = make()
        assert np.array_equal(a1, a2) and np.array_equal(b1, b2) and a1.dtype == np.float32
        assert a1.size // 3 + b1.size // 3 <= 2000
    for f in (GOLD / "chamfer").glob("*.npz"):
        total += f.stat().st_size
    assert total < 100 * 1024


def test_entry_point_and_helpers_do_not_open_the_library(tmp_path):
    code = ("import sys; from neuma_amd import particle_evaluation as pe; pe.parse_args(['-p', 'a']); "
            "pe.group_frames([(1, 2)]); import neuma_amd._lib as L; assert L._lib is None; "
            "assert 'neuma_amd.particle_metrics' not in sys.modules")
    p = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
