"""Two-expert denoising on the host: the (first, last, expert) plan of vstyler.experts over the two
schedules the GPU tests use, the boundary's edge cases, the per-expert guidance pair, and the nearest
source index of vs_resize_nearest_u8 against F.interpolate(mode="nearest")."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import wan_oracle as O
from oracle.unipc_oracle import UniPCOracle
from vstyler.experts import expert_cfg_scales, nearest_index, plan_experts


def euler_timesteps():
    return O.set_timesteps(4, 1.0, 5.0)[1]


def unipc_timesteps():
    s = UniPCOracle(shift=1.0)
    s.set_timesteps(6, shift=2.0)
    return s.timesteps


def test_the_two_schedules():
    te, tu = euler_timesteps(), unipc_timesteps()
    assert te.dtype == torch.float32 and [round(float(t), 2) for t in te] == [1000.0, 937.5, 833.33, 625.0]
    assert tu.dtype == torch.int64 and tu.tolist() == [999, 908, 799, 666, 499, 285]
    assert plan_experts(te, 0.875, True) == [(0, 1, 1), (2, 3, 2)]
    assert plan_experts(tu, 0.875, True) == [(0, 1, 1), (2, 5, 2)]
    assert plan_experts(tu, 0.5, True) == [(0, 3, 1), (4, 5, 2)]
    assert plan_experts(tu[3:], 0.5, True) == [(0, 0, 1), (1, 2, 2)]
    # the product schedulers give the same plans
    from vstyler.flow_match import FlowMatchScheduler
    from vstyler.unipc import FlowUniPCMultistepScheduler
    fm = FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
    fm.set_timesteps(4, denoising_strength=1.0, shift=5.0)
    assert torch.equal(fm.timesteps, te)
    up = FlowUniPCMultistepScheduler(shift=1.0)
    up.set_timesteps(6, shift=2.0)
    assert torch.equal(up.timesteps, tu)
    fm.set_timesteps(3, denoising_strength=0.6, shift=5.0)
    assert [round(float(t)) for t in fm.timesteps] == [882, 769, 556]
    assert plan_experts(fm.timesteps, 0.8, True) == [(0, 0, 1), (1, 2, 2)]


def test_boundary_edges():
    te = euler_timesteps()
    assert float(te[1]) == 937.5
    assert plan_experts(te, 0.9375, True) == [(0, 1, 1), (2, 3, 2)]       # 937.5 is not strictly below
    assert plan_experts(te, 1.0, True) == [(0, 0, 1), (1, 3, 2)]          # 1000 is not below 1000
    assert plan_experts(te, 0, True) == [(0, 3, 1)]
    assert plan_experts(te, 0.0, True) == [(0, 3, 1)]
    assert plan_experts(te, 1.001, True) == [(0, 3, 2)]
    for b in (0, 0.5, 0.875, 1.0, 1.001, 7):
        assert plan_experts(te, b, False) == [(0, 3, 1)]
        assert plan_experts(unipc_timesteps(), b, False) == [(0, 5, 1)]
    assert plan_experts([], 0.875, True) == []
    assert plan_experts([500], 0.875, True) == [(0, 0, 2)]


def test_the_switch_is_sticky():
    """A (hypothetical) schedule that rises again stays on expert 2, as the reference's assignment does."""
    assert plan_experts([900.0, 800.0, 950.0, 100.0], 0.875, True) == [(0, 0, 1), (1, 3, 2)]


def test_segments_cover_every_step_once():
    tu = unipc_timesteps()
    for b in (0.0, 0.3, 0.5, 0.7, 0.875, 0.95, 1.0, 2.0):
        segs = plan_experts(tu, b, True)
        steps = [i for first, last, _ in segs for i in range(first, last + 1)]
        assert steps == list(range(len(tu)))
        for first, last, e in segs:
            for i in range(first, last + 1):
                assert (e == 2) == (float(tu[i]) < b * 1000)


def test_cfg_scale_pair():
    assert expert_cfg_scales(5.0, False) == (5.0, 5.0)
    assert expert_cfg_scales(5, True) == (5.0, 5.0)
    assert expert_cfg_scales(np.float32(1.5), False) == (1.5, 1.5)
    assert expert_cfg_scales((3.0, 4.0), True) == (4.0, 3.0)               # dit: high noise [1]; dit2: [0]
    assert expert_cfg_scales([3, 4.5], True) == (4.5, 3.0)
    with pytest.raises(ValueError, match="second expert"):
        expert_cfg_scales((3.0, 4.0), False)
    for bad in ((3.0,), (1.0, 2.0, 3.0), "5", ("3", "4"), None, (3.0, None), True, (True, 2.0), {"a": 1},
                torch.tensor([3.0, 4.0])):
        with pytest.raises(ValueError, match="cfg_scale"):
            expert_cfg_scales(bad, True)


def test_nearest_index_equals_torch_interpolate():
    """Every (in, out) pair up to 64: the index table against F.interpolate(mode="nearest") of a ramp
    along each axis (CPU float tensors)."""
    for n_in in range(1, 65):
        ramp = torch.arange(n_in, dtype=torch.float32)
        for n_out in range(1, 65):
            idx = nearest_index(n_in, n_out)
            assert idx.dtype == np.int32 and idx.shape == (n_out,)
            rows = F.interpolate(ramp.reshape(1, 1, n_in, 1), size=(n_out, 1), mode="nearest").reshape(-1)
            cols = F.interpolate(ramp.reshape(1, 1, 1, n_in), size=(1, n_out), mode="nearest").reshape(-1)
            assert np.array_equal(idx, rows.numpy().astype(np.int32)), (n_in, n_out)
            assert np.array_equal(idx, cols.numpy().astype(np.int32)), (n_in, n_out)


def test_resize_kernel_rejects_bad_arguments_before_launch():
    from vstyler import _lib
    lib = _lib.load()
    f = 1 << 20             # never dereferenced: validation fails first
    ok = dict(src=f, dst=f + 4096, t=2, h=6, w=10, ho=9, wo=16, c=3)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.vs_resize_nearest_u8(a["src"], a["dst"], a["t"], a["h"], a["w"], a["ho"], a["wo"], a["c"], None)
    for bad in (dict(src=None), dict(dst=None), dict(t=0), dict(h=0), dict(w=0), dict(ho=0), dict(wo=0), dict(t=-1),
                dict(wo=-16), dict(c=1), dict(c=4), dict(c=0)):
        assert call(**bad) == 1, bad
    assert lib.vs_abi_version() == 2
