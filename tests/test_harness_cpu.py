"""Host logic that runs without a GPU: stripe planning, LoRA module semantics, synthetic generator, builders,
and the multi-rank gradient merge over gloo (world_size 2)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp


def test_stripe_plan_partitions_all_rows_exactly_once():
    from neuma_amd.harness import stripe_plan
    for V, rows, world in [(3, 68, 2), (3, 68, 8), (1, 16, 8), (1, 5, 8), (2, 7, 3)]:
        seen = np.zeros((V, rows), dtype=int)
        for r in range(world):
            for (v, a, b) in stripe_plan(V, rows, world, r):
                assert 0 <= a < b <= rows
                seen[v, a:b] += 1
        assert (seen == 1).all()


def test_lora_module_semantics_match_loralib():
    from neuma_amd.material.loralib import LinearLoRA, init_linear_lora, lora_state_dict, mark_only_lora_as_trainable
    torch.manual_seed(0)
    lin = torch.nn.Linear(13, 64, bias=False)
    l = init_linear_lora(lin, r=16, lora_alpha=16)
    assert torch.equal(l.weight, lin.weight) and not l.weight.requires_grad
    assert float(l.lora_B.abs().sum()) == 0 and l.scaling == 1.0
    l.lora_B.data.normal_()
    x = torch.randn(5, 13)
    y = l(x)
    assert torch.allclose(y, x @ l.effective_weight().T, atol=1e-5)
    w0 = l.weight.clone()
    l.eval()
    assert l.merged and torch.allclose(l.weight, w0 + l.lora_B @ l.lora_A)
    assert torch.allclose(l(x), y, atol=1e-5) and torch.equal(l.effective_weight(), l.weight)
    l.train()
    assert not l.merged and torch.allclose(l.weight, w0, atol=1e-6)
    m = torch.nn.Sequential(l)
    mark_only_lora_as_trainable(m)
    assert sorted(lora_state_dict(m).keys()) == ["0.lora_A", "0.lora_B"]


def test_material_module_tree_loads_reference_checkpoint_keys(golden_dir):
    from neuma_amd.material import InvariantFullMetaElasticity, InvariantFullMetaPlasticity
    b = np.load(golden_dir / "base_models.npz")
    cfg = dict(layer_widths=[64, 64], norm=None, nonlinearity="gelu", no_bias=True, normalize_input=True, alpha=1e-3)
    for cls, t in ((InvariantFullMetaElasticity, "e"), (InvariantFullMetaPlasticity, "p")):
        net = cls(cfg)
        sd = {"layers.0.fc.weight": torch.tensor(b[f"jelly_{t}_w0"]), "layers.1.fc.weight": torch.tensor(b[f"jelly_{t}_w1"]),
              "final_layer.fc.weight": torch.tensor(b[f"jelly_{t}_w2"])}
        assert set(net.state_dict().keys()) == set(sd.keys())
        net.load_state_dict(sd)
        net.init_lora_layers(16, 16)
        net.freeze_all_except_lora()
        assert sorted(net.lora_state_dict().keys()) == sorted(
            f"{p}.fc.lora_{ab}" for p in ("layers.0", "layers.1", "final_layer") for ab in "AB")
        assert [tuple(w.shape) for w in net.effective_weights()] == [(64, 13), (64, 64), (9, 64)]
    with pytest.raises(NotImplementedError):
        InvariantFullMetaElasticity(dict(cfg, layer_widths=[32, 32]))


def test_builder_and_initializers_on_cpu():
    from neuma_amd.sim import MPMModelBuilder, MPMInitData, MPMStateInitializer, MPMStaticsInitializer
    cfg = dict(gravity=[0, -9.8, 0], bc="noslip", num_grids=32, dt=1e-3, bound=1, eps=0.0)
    model = MPMModelBuilder().parse_cfg(cfg).finalize("cpu")
    assert model.constant.dx == 1 / 32 and model.constant.inv_dx == 32.0
    rng = np.random.default_rng(0)
    pts = rng.random((100, 3)) - np.array([0.5, 0.0, 0.5])
    kw = MPMInitData.from_points(pts, 1e-6, [[-0.5, 0, -0.5], [0.5, 1, 0.5]], [[0.2, 0.2, 0.2], [0.8, 0.8, 0.8]])
    g1 = MPMInitData(rho=1000.0, clip_bound=0.1, span=(0, 10), **kw)
    g2 = MPMInitData(rho=500.0, clip_bound=0.2, span=(5, 20), **kw)
    g2.set_lin_vel([1.0, 0, 0])
    si = MPMStateInitializer(model); si.add_group(g1); si.add_group(g2)
    state, sections = si.finalize()
    assert sections == [100, 100] and state.particle.x.shape == (200, 3)
    assert torch.allclose(state.particle.v[100:, 0], torch.ones(100))
    sti = MPMStaticsInitializer(model); sti.add_group(g1); sti.add_group(g2)
    st = sti.finalize()
    assert st.enabled[:100].all() and not st.enabled[100:].any()          # span (5,20) disabled at step 0
    sti.update(st, step=7)
    assert st.enabled.all()
    sti.update(st, step=12)
    assert not st.enabled[:100].any() and st.enabled[100:].all()
    assert float(st.rho[150]) == 500.0 and abs(float(st.vol[0]) - kw["vol"]) < 1e-12


def test_initializers_match_the_reference_run(golden_dir):
    """mpm_init.npz was produced by running the reference's MPMStateInitializer / MPMStaticsInitializer / update_enabled /
    alignment / builder themselves (tests/golden/gen_mpm_golden.py, gen_init)."""
    from neuma_amd.sim import MPMModelBuilder, MPMInitData, MPMStateInitializer, MPMStaticsInitializer
    z = np.load(golden_dir / "mpm_init.npz")
    model = MPMModelBuilder().parse_cfg(dict(gravity=[0.0, -9.8, 0.0], bc="noslip", num_grids=8, dt=1e-3, bound=1, eps=6e-7)).finalize("cpu")
    c = model.constant
    assert np.allclose([c.num_grids, c.dt, c.bound, c.dx, c.inv_dx, c.eps, *np.asarray(c.gravity)], z["constant"], rtol=1e-7, atol=0)
    si, sti = MPMStateInitializer(model), MPMStaticsInitializer(model)
    for i in range(3):
        rho, clip, s0, s1, vol, *vel = z[f"spec_{i}"]
        g = MPMInitData(rho=float(rho), clip_bound=float(clip), span=(int(s0), int(s1)), num_particles=len(z[f"pos_{i}"]), vol=float(vol),
                        pos=z[f"pos_{i}"], lin_vel=np.array(vel[:3]), ang_vel=np.array(vel[3:]))
        if i == 1:
            g.set_ind_vel(z["ind_vel_1"])
        si.add_group(g); sti.add_group(g)
    state, sections = si.finalize()
    st = sti.finalize()
    assert sections == list(z["sections"])
    for name in ["x", "v", "C", "F"]:
        assert np.array_equal(getattr(state.particle, name).numpy(), z[name]), name      # fp32 cast of the same fp64 values
    for name in ["vol", "rho", "clip_bound"]:
        assert np.array_equal(getattr(st, name).numpy(), z[name]), name
    for step in [0, 2, 3, 4, 5, 999, 1000]:
        sti.update(st, step)
        assert np.array_equal(st.enabled.numpy(), z[f"enabled_{step}"]), step
    s, t = MPMInitData.alignment(np.array([-1.0, -2.0, 0.0]), np.array([1.0, 2.0, 4.0]), np.array([0.3, 0.3, 0.3]), np.array([0.7, 0.6, 0.5]))
    assert np.allclose(s, z["align_scale"], rtol=1e-15) and np.allclose(t, z["align_trans"], rtol=1e-15, atol=1e-16)


def test_synth_scene_is_deterministic_and_in_bounds():
    from neuma_amd import synth
    a, b = synth.make_scene("tiny"), synth.make_scene("tiny")
    assert np.array_equal(a.x0, b.x0) and np.array_equal(a.bind_idx, b.bind_idx)
    assert a.x0.min() > 0 and a.x0.max() < 1 and a.bind_idx.max() < a.x0.shape[0]
    from neuma_amd.tune import Bindings
    K, nb = a.bind_idx.shape
    ind = torch.stack([torch.arange(K).repeat_interleave(nb), torch.tensor(a.bind_idx.reshape(-1))])
    bd = Bindings(ind, torch.tensor(a.bind_w.reshape(-1)), (K, a.x0.shape[0]), "cpu")
    dense = torch.zeros(K, a.x0.shape[0]).index_put_((ind[0], ind[1]), torch.tensor(a.bind_w.reshape(-1)), accumulate=True)
    # CSR and transposed CSR describe the same matrix
    rp, col, val = bd.rowptr.long(), bd.col.long(), bd.val
    rec = torch.zeros_like(dense)
    for r in range(0, K, 97):
        rec[r].index_add_(0, col[rp[r]:rp[r + 1]], val[rp[r]:rp[r + 1]])
        assert torch.allclose(rec[r], dense[r])
    tp, tcol, tval = bd.t_rowptr.long(), bd.t_col.long(), bd.t_val
    for c in range(0, a.x0.shape[0], 131):
        colv = torch.zeros(K).index_add_(0, tcol[tp[c]:tp[c + 1]], tval[tp[c]:tp[c + 1]])
        assert torch.allclose(colv, dense[:, c])


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _rank_main(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from neuma_amd.harness import merge_grad_across_ranks, stripe_plan
    torch.manual_seed(0)
    K, V, rows = 50, 3, 10
    means = torch.randn(K, 3, requires_grad=True)          # replicated "simulation output"
    m = merge_grad_across_ranks(means)
    W = torch.randn(V, rows, K, 3)                          # stand-in for per-(view,row) render+loss pieces
    loss = sum((W[v, a:b].sum(0) * m).sum() for (v, a, b) in stripe_plan(V, rows, world, rank))
    loss.backward()
    full = W.sum((0, 1))
    tot = torch.tensor([float(loss)]); dist.all_reduce(tot)
    q.put((rank, bool(torch.allclose(means.grad, full, atol=1e-4)), float(tot), float((full * means.detach()).sum())))
    dist.destroy_process_group()


def test_two_rank_gloo_gradient_merge_equals_single_rank():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_rank_main, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in ps]
    res = [q.get(timeout=120) for _ in ps]
    [p.join(30) for p in ps]
    for rank, ok, tot, ref in res:
        assert ok, f"rank {rank}: merged gradient differs from the single-rank gradient"
        assert abs(tot - ref) < 1e-3 * max(1.0, abs(ref))


def test_lr_schedulers_match_reference_curves(golden_dir):
    """neuma_amd.train schedulers vs curves produced by the reference's modules/tune/scheduler (gen_material_golden.py)."""
    from neuma_amd.train import fetch_scheduler, rollout_decay_rate
    g = np.load(golden_dir / "scheduler_golden.npz")
    for tag, cfgd, lr0 in [("cos", dict(type="cos", max_steps=1000, learning_rate_alpha=0.025), 0.008),
                           ("cos_warm", dict(type="cos", max_steps=200, learning_rate_alpha=0.01, warm_up_end=20), 1.0),
                           ("exp", dict(type="exp", lr_final=1e-4, max_steps=500, warmup_steps=10), 0.01)]:
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([p], lr=lr0)
        sc = fetch_scheduler(cfgd).get_scheduler(opt, lr0)
        lrs = []
        for _ in range(int(cfgd["max_steps"]) + 5):
            lrs.append(opt.param_groups[0]["lr"])
            opt.step(); sc.step()
        assert np.allclose(np.array(lrs), g[tag], rtol=1e-12, atol=1e-15), tag
    with pytest.raises(ValueError):
        fetch_scheduler(dict(type="step"))
    c = dict(decay_init=0.5, decay_final=1.0, lambda_max_decay=0.33, num_epochs=1000)
    assert rollout_decay_rate(c, 0) == 0.5 and rollout_decay_rate(c, 1000) == 1.0      # finetune.py:353-358
    assert abs(rollout_decay_rate(c, 165) - (0.5 + 0.5 * (165 / 0.33 / 1000))) < 1e-12
    assert rollout_decay_rate(dict(c, lambda_max_decay=0), 3) == 1.0


def test_finetune_loop_accumulates_gradients_like_the_reference(tmp_path, monkeypatch):
    """experiments/finetune.py:331-484 never zeroes the LoRA gradients: `.grad` adds up over the epochs before clip + RAdam.
    Host control flow only - the video loss is replaced by a closed-form function of the LoRA parameters."""
    from types import SimpleNamespace
    from torch.optim import RAdam
    from torch.nn.utils import clip_grad_norm_
    from neuma_amd import train
    from neuma_amd.material import InvariantFullMetaElasticity, InvariantFullMetaPlasticity
    cfg = dict(layer_widths=[64, 64], norm=None, nonlinearity="gelu", no_bias=True, normalize_input=True, alpha=1e-3)

    def nets():
        torch.manual_seed(3)
        E, P = InvariantFullMetaElasticity(cfg), InvariantFullMetaPlasticity(cfg)
        for n in (E, P):
            n.init_lora_layers(16, 16)
            for lin in (n.layers[0].fc, n.layers[1].fc, n.final_layer.fc):
                lin.lora_B.data.normal_(0, 0.01)
        return E, P

    def fake_loss(rt, gt, c, decay, views, **kw):
        return sum(((p - 0.01 * (i + 1)) ** 2).sum() * decay for i, p in enumerate(rt.parameters_()))

    monkeypatch.setattr(train, "video_loss", fake_loss)
    c = dict(num_epochs=4, num_frames=1, elasticity_lr=0.01, plasticity_lr=0.01, elasticity_grad_max_norm=50.0,
             plasticity_grad_max_norm=50.0, elasticity_scheduler=dict(type="cos", max_steps=4, learning_rate_alpha=0.1),
             plasticity_scheduler=dict(type="cos", max_steps=4, learning_rate_alpha=0.1))
    out = {}
    for acc in (True, False):
        E, P = nets()
        rt = SimpleNamespace(elasticity=E, plasticity=P, V=1, device="cpu")
        rt.parameters_ = lambda E=E, P=P: [p for n in (E, P) for p in n.parameters() if p.requires_grad]
        train.finetune_constitutive(rt, None, dict(c, accumulate_grads_like_reference=acc), tune_root=tmp_path / str(acc))
        out[acc] = [p.detach().clone() for p in rt.parameters_()]
        # hand-rolled loop with the same optimiser settings
        E2, P2 = nets()
        E2.freeze_all_except_lora(); P2.freeze_all_except_lora()
        ps = [p for n in (E2, P2) for p in n.parameters() if p.requires_grad]
        eo = RAdam([p for p in E2.parameters() if p.requires_grad], lr=0.01)
        po = RAdam([p for p in P2.parameters() if p.requires_grad], lr=0.01)
        es = train.fetch_scheduler(c["elasticity_scheduler"]).get_scheduler(eo, 0.01)
        psch = train.fetch_scheduler(c["plasticity_scheduler"]).get_scheduler(po, 0.01)
        for epoch in range(1, 5):
            decay = train.rollout_decay_rate(dict(train.DEFAULT_CFG, **c), epoch)
            if not acc:
                eo.zero_grad(); po.zero_grad()
            sum(((p - 0.01 * (i + 1)) ** 2).sum() * decay for i, p in enumerate(ps)).backward()
            clip_grad_norm_(E2.parameters(), 50.0); eo.step()
            clip_grad_norm_(P2.parameters(), 50.0); po.step()
            es.step(); psch.step()
        for a, b in zip(out[acc], ps):
            assert torch.allclose(a, b, atol=1e-7), acc
    assert any(not torch.allclose(a, b, atol=1e-6) for a, b in zip(out[True], out[False]))      # the two behaviours do differ
    names = sorted(p.name for p in (tmp_path / "True").glob("*_lora.pt"))
    assert names == ["0001_lora.pt", "0004_lora.pt"]


def test_checkpoint_order_is_by_epoch_number(tmp_path):
    from neuma_amd.train import lora_checkpoints
    for e in (9990, 10000, 1, 10):
        (tmp_path / f"{e:04d}_lora.pt").write_bytes(b"")
    assert [p.name for p in lora_checkpoints(tmp_path)] == ["0001_lora.pt", "0010_lora.pt", "9990_lora.pt", "10000_lora.pt"]


def test_cache_pool_accounting_per_device_trim_and_retry(monkeypatch):
    """neuma_amd.rollout's cache pool (host logic, CPU tensors): live bytes are counted per device, idle buffers go back to the
    pool and trim_pool() drops them, and an allocation that fails trims the pool and retries once before the node falls back to
    recomputing (one global counter, no way to give the pooled GB back)."""
    from neuma_amd import rollout as R
    monkeypatch.setattr(R, "_BUDGET", {"cpu": 1 << 20, "meta": 1 << 20})
    monkeypatch.setattr(R, "_POOL", {})
    monkeypatch.setattr(R, "_ACT_LIVE", {})
    a = R.lease_cache(1000, "cpu")
    b = R.lease_cache(3000, "cpu")
    assert R.live_bytes("cpu") == 4000 and R.live_bytes("meta") == 0 and R.live_bytes() == 4000
    assert R.lease_cache(1 << 21, "cpu") is None                      # over the device's budget: the node recomputes
    a.release(); b.release()
    assert R.live_bytes("cpu") == 0 and sum(len(v) for v in R._POOL.values()) == 2
    c = R.lease_cache(1000, "cpu")                                    # comes out of the pool
    assert sum(len(v) for v in R._POOL.values()) == 1 and c.t.numel() == 1000
    c.release()
    assert R.trim_pool("cpu") == 4000 and R._POOL == {}
    # an allocation that fails: pool trimmed, one retry; still failing -> None (force: the error surfaces)
    R.lease_cache(2000, "cpu").release()
    calls = {"n": 0}
    real_empty = torch.empty

    def failing_empty(*args, **kw):
        calls["n"] += 1
        if calls["n"] <= fail_first:
            raise torch.cuda.OutOfMemoryError("simulated")
        return real_empty(*args, **kw)

    monkeypatch.setattr(torch, "empty", failing_empty)
    fail_first = 1
    d = R.lease_cache(5000, "cpu")
    assert d is not None and calls["n"] == 2 and R._POOL == {}        # (the idle 2000-byte buffer was given back before the retry)
    d.release()
    R.trim_pool()
    calls["n"], fail_first = 0, 2
    assert R.lease_cache(5000, "cpu") is None and R.live_bytes("cpu") == 0
    calls["n"] = 0
    with pytest.raises(torch.cuda.OutOfMemoryError):
        R.lease_cache(5000, "cpu", force=True)


class _StubEvent(object):
    """query() / synchronize() of torch.cuda.Event; `after_sync`: what query() says once synchronize() has been called."""

    def __init__(self, done, after_sync=True):
        self.done, self.after_sync, self.syncs = done, after_sync, 0

    def query(self):
        return self.done

    def synchronize(self):
        self.syncs += 1
        self.done = self.after_sync


class _StubSizes(object):
    """The four size queries of the roll-out (any lib object with these serves RolloutCall.open)."""
    nm_rollout_workspace = staticmethod(lambda n, S: 64 * n)
    nm_rollout_gridcache_bytes = staticmethod(lambda S, blocks: 16 * S * blocks)
    nm_rollout_svdcache_bytes = staticmethod(lambda n, S: 168 * n * S)
    nm_rollout_actcache_bytes = staticmethod(lambda n, S: 1200 * n * S)


def test_rollout_call_builds_both_halves_of_the_protocol_from_one_record(monkeypatch):
    """neuma_amd.rollout.RolloutCall (host logic, CPU tensors): the forward and the reverse nm_rollout_cfg of each of the three
    drivers (autograd node, lean frame, native epoch) agree on every field the library compares; cache_verified follows ONE rule -
    1 only when the status words have landed (the event has completed) and none is negative; close() returns both leases and
    the pooled status words, once."""
    from neuma_amd import rollout as R
    monkeypatch.setattr(R, "_BUDGET", {"cpu": 1 << 30})
    monkeypatch.setattr(R, "_POOL", {})
    monkeypatch.setattr(R, "_ACT_LIVE", {})
    monkeypatch.setattr(R, "_SIZES", {})
    monkeypatch.setattr(R, "_SVD_CACHE", True)
    monkeypatch.setattr(R, "_ACT_CACHE", "auto")
    monkeypatch.setattr(R, "_CACHE_WAIT", True)
    lib, n, S = _StubSizes(), 10, 4
    shared = ("substeps", "plasticity_alpha", "grid_cache_blocks", "svd_adjoint", "svd_cache", "act_cache")
    pool = []
    drivers = {     # name -> (open keywords, backward_cfg keywords, does the driver promise the same last_gF_zero in both halves)
        "node": (dict(want_backward=True), dict(last_gF_zero=1), False),
        "node, dL/dF arrives": (dict(want_backward=True), dict(last_gF_zero=0), True),
        "frame": (dict(last_gF_zero=1, status_pool=pool), dict(weights_prepared=1, last_gF_zero=1), True),
        "frame, NEUMA_LAST_GF_ZERO=0": (dict(last_gF_zero=0, status_pool=pool), dict(weights_prepared=0, last_gF_zero=0), True),
        "epoch, last frame": (dict(last_gF_zero=1), dict(last_gF_zero=1), True),
        "epoch, earlier frame": (dict(last_gF_zero=0), dict(last_gF_zero=0), True),
        "epoch, word left to the call": (dict(last_gF_zero=1), dict(), True),
    }
    for name, (okw, bkw, same_word) in drivers.items():
        call = R.RolloutCall.open(lib, "cpu", n, S, 1e-3, 1, 7, **okw)
        assert call.ws_bytes == 64 * n and call.gcache.numel() == 16 * S * 7 and call.svdc is not None and call.actc is not None, name
        assert R.live_bytes("cpu") == (168 + 1200) * n * S, name
        fwd = call.forward_cfg()
        call.status, call.event = torch.zeros(S, dtype=torch.int32), _StubEvent(True)      # (what watch() leaves behind on a GPU)
        bwd = call.backward_cfg(**bkw)
        for k in shared:
            assert getattr(fwd, k) == getattr(bwd, k), (name, k)
        assert (fwd.substeps, fwd.grid_cache_blocks, fwd.svd_adjoint) == (S, 7, 1) and abs(fwd.plasticity_alpha - 1e-3) < 1e-9, name
        assert fwd.svd_cache == call.svdc.t.data_ptr() and fwd.act_cache == call.actc.t.data_ptr(), name
        assert (fwd.cache_verified, fwd.weights_prepared, bwd.cache_verified) == (0, 0, 1), name
        assert bwd.weights_prepared == bkw.get("weights_prepared", 0), name
        assert fwd.last_gF_zero == okw.get("last_gF_zero", 0) and bwd.last_gF_zero == bkw.get("last_gF_zero", fwd.last_gF_zero), name
        assert (fwd.last_gF_zero == bwd.last_gF_zero) or not same_word, name
        call.close()
        assert R.live_bytes("cpu") == 0 and sum(len(v) for v in R._POOL.values()) == 2, name
        assert call.gcache is None and call.svdc is None and call.actc is None and call.status is None and call.event is None, name
        call.close()                                                      # a second close() is a no-op
        assert R.live_bytes("cpu") == 0 and sum(len(v) for v in R._POOL.values()) == 2, name
        assert len(pool) == (1 if "status_pool" in okw else 0), name      # the landed words went back to the pool, once
        pool.clear()
    # no backward pass can follow (ground truth, inference): no caches, nothing leased, nothing to verify
    call = R.RolloutCall.open(lib, "cpu", n, S, 1e-3, 0, 7, want_backward=False)
    cfg = call.backward_cfg()
    assert call.gcache is None and (cfg.grid_cache_blocks, cfg.cache_verified, cfg.svd_cache, cfg.act_cache) == (0, 0, None, None)
    assert R.live_bytes("cpu") == 0
    # verified(): the words are read only once the event has completed
    words_ok, words_bad = torch.zeros(S, dtype=torch.int32), torch.tensor([0, 3, -1, 0], dtype=torch.int32)
    call = R.RolloutCall.open(lib, "cpu", n, S, 1e-3, 0, 7, status_pool=pool)
    assert call.verified() == 0                                           # nothing was watched
    call.status, call.event = words_ok, _StubEvent(False)
    assert call.verified() == 1 and call.event.syncs == 1                 # NEUMA_CACHE_WAIT=1 (default): the host waits for the words
    call.status, call.event = words_bad, _StubEvent(True)
    assert call.verified() == 0 and call.backward_cfg().cache_verified == 0      # a negative word: a record is not valid
    monkeypatch.setattr(R, "_CACHE_WAIT", False)
    call.landed = False
    call.status, call.event = words_bad, _StubEvent(False)
    assert call.verified() == 0 and call.event.syncs == 0 and not call.landed
    call.status = words_ok                                                # event incomplete: 0 whatever the (unwritten) words say
    assert call.verified() == 0 and call.backward_cfg().cache_verified == 0 and not call.landed
    call.close()
    assert pool == [] and R.live_bytes("cpu") == 0                        # words still in flight are not handed back
    call = R.RolloutCall.open(lib, "cpu", n, S, 1e-3, 0, 7, status_pool=pool)
    call.status, call.event = words_ok, _StubEvent(True)
    assert call.verified() == 1 and call.event.syncs == 0
    call.close()
    assert len(pool) == 1 and pool[0][0] is words_ok
    # the packed weight buffer and the LoRA gradient jobs
    from neuma_amd import _lib as L
    nw = sum(R._WSZ)
    mle, mlp = R.mlp_pair(1000, nw)
    assert (mle.w0, mle.w1, mle.w2) == (1000, 1000 + 4 * R._WSZ[0], 1000 + 4 * (R._WSZ[0] + R._WSZ[1]))
    assert (mlp.w0, mlp.w1, mlp.w2) == tuple(p + 4 * nw for p in (mle.w0, mle.w1, mle.w2))
    jb = (L.nm_lora_layer * 6)()
    woff, goff, sizes = [0, 10, 30, 60, 100, 150], [0, 5, 12, 21, 32, 45], [2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8]
    R.lora_grad_jobs(jb, 8000, 16000, woff, goff, sizes)
    for i in range(6):
        assert (jb[i].W, jb[i].o0, jb[i].o1) == (8000 + 4 * woff[i], 16000 + 4 * goff[i], 16000 + 4 * (goff[i] + sizes[2 * i]))


def test_inference_entry_point_reads_the_reference_demo_configs(golden_dir):
    """`python -m neuma_amd.inference`: its argument parser mirrors experiments/inference.py:48-84 and the loader turns the four
    shipped demo YAMLs into what `inference()` consumes (objects, per-object checkpoints / adaptors / velocities, sim block).
    The YAMLs are the reference's experiments/configs/demo/*.yaml, stored unchanged under tests/golden/demo_configs/."""
    from neuma_amd.config import load_config
    from neuma_amd.inference import parse_args
    a = parse_args(["-c", "x.yaml", "-vn", "clip", "-s", "50", "-dv", "e_2", "e_3", "-sp", "run", "-f", "5", "-ri"])
    assert (a.config, a.video_name, a.eval_steps, a.debug_views, a.save_particles, a.skip_frames, a.remove_images) == \
        ("x.yaml", "clip", 50, ["e_2", "e_3"], "run", 5, True)
    d = parse_args(["-c", "x.yaml", "-vn", "clip"])
    assert d.eval_steps == 600 and d.debug_views == [] and d.save_particles is None and d.dataset_path is None      # inference.py:54-81
    seen = 0
    for f in sorted((golden_dir / "demo_configs").glob("*.yaml")):
        c = load_config(f)
        assert len(c.objects) >= 1 and c.sim.num_grids > 0 and c.sim.bc in ("noslip", "freeslip")
        for o in c.objects:
            assert o.pretrained_ckpt.endswith("_0300.pt") and o.constitution.lora.r == 16 and o.constitution.load_lora.endswith("_lora.pt")
            assert len(o.particle_data.vel.lin_vel) == 3 and len(o.particle_data.shape.sim_bounds) == 2
            assert o.constitution.elasticity.layer_widths == [64, 64] and o.gaussian.sh_degree in (0, 3)
        seen += 1
    assert seen == 4
