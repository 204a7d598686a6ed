"""Temporal sliding window on the GPU: vs_window_blend / vs_window_finish bit-exact against the torch
expression of TemporalTiler_BCTHW (wan_video_new.py:1252-1254) on bf16 tensors, and the windowed
model_fn_wan_video / WanVideoPipeline / denoise_unipc bit-exact against a test-side tiler
(tests/window_util.py) around the plain product forward, and within the oracle's floor against the
same tiler around O.model_fn.  Tiny config, 64x96, 33 frames (T = 9 latent frames of 24 tokens)."""
import pytest
import torch

from gpu_util import err
from oracle import wan_oracle as O
from test_model_gpu import build
from test_sp import _init, _spawn
from window_util import tile, tiled_model_fn

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
H, WD, FRAMES, T = 64, 96, 33, 9
WINDOWS = [(5, 3), (5, 2)]


def bits(t):
    return t.cpu().contiguous().view(torch.int16)


def _rand_bf16(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g).to(BF16)
    x[0::5] = 0.0
    x[2::7] = -0.0
    return x


# ------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("hw", [(2, 2), (6, 10), (8, 12), (3, 5)])
@pytest.mark.parametrize("T_,size,stride", [(9, 5, 2), (9, 5, 3), (9, 4, 1)])
def test_window_kernels_bit_exact(hw, T_, size, stride):
    """BC = 2*16.  Planes 4 and 60 put window bases (t0 > 0, and every other row at T = 9) 4 elements
    off a 16-byte boundary in `value` and, for the 3-frame ragged window of plane 4 / 60, in `out`; 96
    keeps everything aligned; 15 (odd, beyond what the pipeline produces) reaches every misalignment.
    (9, 5, 2): triple overlap at frame 4 with the overwritten ramp; (9, 5, 3): ragged last window;
    (9, 4, 1): six windows."""
    from vstyler import kernels as K
    from vstyler.window import plan_windows
    h, w = hw
    B, C = 2, 16
    plan = plan_windows(T_, size, stride)
    outs = [_rand_bf16(B * C * (t_ - t) * h * w, 10 + i).roll(i).reshape(B, C, t_ - t, h, w)
            for i, (t, t_) in enumerate(plan.windows)]
    value = torch.zeros((B, C, T_, h, w), dtype=BF16)
    weight = torch.zeros((1, 1, T_, 1, 1), dtype=BF16)
    for (t, t_), m, out in zip(plan.windows, plan.masks, outs):
        mask = m.reshape(1, 1, -1, 1, 1)
        value[:, :, t:t_] += out * mask
        weight[:, :, t:t_] += mask
    assert torch.equal(bits(weight.reshape(-1)), bits(plan.weight))
    blended = value.clone()
    value /= weight

    vd = torch.zeros((B, C, T_, h, w), dtype=BF16, device="cuda")
    for (t, t_), m, out in zip(plan.windows, plan.masks, outs):
        od = out.cuda()
        assert K.window_blend(od, m.cuda(), vd, t) is vd
        assert torch.equal(bits(od), bits(out)), "out was written"
    assert torch.equal(bits(vd), bits(blended))
    wd = plan.weight.cuda()
    res = torch.full_like(vd, 7.0)
    assert K.window_finish(vd, wd, out=res) is res
    assert torch.equal(bits(res), bits(value))
    assert torch.equal(bits(vd), bits(blended)), "value was written by the out-of-place finish"
    assert K.window_finish(vd, wd) is vd
    assert torch.equal(bits(vd), bits(value))
    assert (value == 0).any() and not torch.signbit(value[value == 0]).any()     # 0 + (-0) = +0 throughout


def test_window_gather_equals_the_slice():
    from vstyler import kernels as K
    x = _rand_bf16(2 * 16 * 9 * 60, 3).reshape(2, 16, 9, 6, 10).cuda()
    for t, t_ in ((0, 5), (3, 8), (6, 9), (8, 9)):
        dst = torch.full((2, 16, t_ - t, 6, 10), 7.0, dtype=BF16, device="cuda")
        assert K.window_gather(x, t, dst) is dst
        assert torch.equal(bits(dst), bits(x[:, :, t:t_]))
    with pytest.raises(ValueError):
        K.window_gather(x, 6, torch.empty((2, 16, 5, 6, 10), dtype=BF16, device="cuda"))


def test_window_kernels_invalid_arguments():
    from vstyler import _lib, kernels as K
    lib = _lib.load()
    f = 1 << 20             # aligned, never dereferenced: validation fails first
    ok = dict(out=f, mask=f, value=f, bc=32, t=9, l=5, t0=3, plane=60)

    def blend(**kw):
        a = dict(ok, **kw)
        return lib.vs_window_blend(a["out"], a["mask"], a["value"], a["bc"], a["t"], a["l"], a["t0"], a["plane"], None)
    for bad in (dict(out=None), dict(mask=None), dict(value=None), dict(bc=0), dict(t=0), dict(l=0), dict(plane=0),
                dict(bc=-1), dict(l=-1), dict(plane=-4), dict(t0=-1), dict(t0=5), dict(l=10, t0=0), dict(out=f + 2),
                dict(value=f + 8), dict(mask=f + 1)):
        assert blend(**bad) == 1, bad
    okf = dict(value=f, weight=f, out=f, bc=32, t=9, plane=60)

    def finish(**kw):
        a = dict(okf, **kw)
        return lib.vs_window_finish(a["value"], a["weight"], a["out"], a["bc"], a["t"], a["plane"], None)
    for bad in (dict(value=None), dict(weight=None), dict(out=None), dict(bc=0), dict(t=0), dict(plane=0),
                dict(t=-9), dict(value=f + 2), dict(out=f + 4), dict(weight=f + 1)):
        assert finish(**bad) == 1, bad
    v = torch.zeros((2, 16, 9, 2, 2), dtype=BF16, device="cuda")
    o = torch.zeros((2, 16, 5, 2, 2), dtype=BF16, device="cuda")
    m = torch.ones(5, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError, match="VS_E_INVALID"):
        K.window_blend(o, m, v, 5)                                  # t0 + L > T
    with pytest.raises(ValueError):
        K.window_blend(o, m[:4], v, 0)
    with pytest.raises(ValueError):
        K.window_blend(o.float(), m, v, 0)
    with pytest.raises(ValueError):
        K.window_blend(o[:, :8], m, v, 0)
    with pytest.raises(ValueError):
        K.window_finish(v, m)
    with pytest.raises(ValueError):
        K.window_finish(v, torch.ones(9, device="cuda"))
    assert not v.any()


# ------------------------------------------------------------------------------------------ model_fn
@pytest.fixture(scope="module")
def tiny():
    from vstyler import WanVideoPipeline
    cfg = O.WAN_CONFIGS["tiny"]
    W = O.random_weights(cfg, seed=5)
    pipe = WanVideoPipeline(device="cuda")
    pipe.dit, pipe.vace = build(cfg, W)
    lat, cp, cn, vc = O.synthetic_inputs(cfg, FRAMES, H, WD)
    assert lat.shape[2] == T
    return cfg, W, pipe, lat, cp, cn, vc


def _timestep():
    return torch.tensor([833.3333]).to(BF16)


def _product(pipe, lat, ctx, vc, **kw):
    from vstyler import model_fn_wan_video
    return model_fn_wan_video(pipe.dit, vace=pipe.vace, latents=lat.cuda(), timestep=_timestep().cuda(),
                              context=ctx.cuda(), vace_context=None if vc is None else vc.cuda(), **kw)


@pytest.mark.parametrize("size,stride", WINDOWS)
def test_windowed_model_fn_equals_the_test_side_tiler(tiny, size, stride):
    """Batch-2 CFG context over shared latents; the windowed forward == the reference's tiler around
    the plain product forward on every [t, t_) slice of the latents and the VACE context, blended with
    torch tensor ops on the device."""
    from vstyler import model_fn_wan_video
    cfg, W, pipe, lat, cp, cn, vc = tiny
    ctx = torch.cat([cp, cn])
    got = _product(pipe, lat, ctx, vc, sliding_window_size=size, sliding_window_stride=stride)
    assert got.shape == (2, 16, T, H // 8, WD // 8) and got.dtype == BF16

    def plain(l, v):
        return model_fn_wan_video(pipe.dit, vace=pipe.vace, latents=l, timestep=_timestep().cuda(),
                                  context=ctx.cuda(), vace_context=v)
    want = tile(plain, lat.cuda(), vc.cuda(), size, stride)
    assert torch.equal(bits(got), bits(want))
    # without a VACE context, and with the context cut by the caller
    assert torch.equal(bits(_product(pipe, lat, ctx, None, sliding_window_size=size, sliding_window_stride=stride)),
                       bits(tile(plain, lat.cuda(), None, size, stride)))
    from vstyler.pipeline import slice_windows
    from vstyler.window import plan_windows
    cut = slice_windows(vc.cuda(), plan_windows(T, size, stride))
    assert torch.equal(bits(_product(pipe, lat, ctx, vc, sliding_window_size=size, sliding_window_stride=stride,
                                     vace_context_windows=cut)), bits(want))
    assert not torch.equal(got, _product(pipe, lat, ctx, vc))      # the windows are not the full forward


@pytest.mark.parametrize("size,stride", WINDOWS)
def test_windowed_model_fn_vs_oracle(tiny, size, stride):
    """The same tiler around O.model_fn, once for each CFG sample; floor: the oracle's fp32 run against
    its fp64-accumulation run; criterion of test_v2v_gpu.test_euler_v2v_vs_oracle_chain."""
    cfg, W, pipe, lat, cp, cn, vc = tiny
    got = _product(pipe, lat, torch.cat([cp, cn]), vc, sliding_window_size=size, sliding_window_stride=stride)

    def run():
        return torch.cat([tile(lambda l, v: O.model_fn(W, cfg, l, _timestep(), c, v), lat, vc, size, stride)
                          for c in (cp, cn)])
    ref = run()
    old = O.ACC_DTYPE
    O.ACC_DTYPE = torch.float64
    try:
        ref64 = run()
    finally:
        O.ACC_DTYPE = old
    fmx, frel = err(ref64, ref)
    mx, rel = err(got, ref)
    print(f"windowed model_fn ({size}, {stride}): max-abs {mx:.4g} rel-L2 {rel:.4g} (floor {fmx:.4g} / {frel:.4g})")
    assert rel <= 1.5 * frel + 2e-3 and mx <= 1.5 * fmx + 2e-2


def test_single_window_is_the_plain_path(tiny):
    cfg, W, pipe, lat, cp, cn, vc = tiny
    ctx = torch.cat([cp, cn])
    plain = _product(pipe, lat, ctx, vc)
    for size, stride in ((T, 3), (T + 3, T + 3), (12, 1)):
        assert torch.equal(bits(_product(pipe, lat, ctx, vc, sliding_window_size=size, sliding_window_stride=stride)),
                           bits(plain)), (size, stride)
    assert torch.equal(bits(_product(pipe, lat, ctx, vc, sliding_window_stride=3)), bits(plain))   # stride alone
    kw = dict(prompt_emb=cp, negative_prompt_emb=cn, vace_context=vc, seed=3, height=H, width=WD, num_frames=FRAMES,
              num_inference_steps=2, output_type="latents")
    assert torch.equal(bits(pipe(sliding_window_size=T, sliding_window_stride=4, **kw)), bits(pipe(**kw)))


def test_workspace_is_stable_across_windowed_forwards(tiny):
    """(5, 3) ends in a ragged 3-frame window: the full and the ragged window's buffers alternate
    inside one forward.  After the first forward a second one moves no buffer and allocates nothing."""
    from vstyler.pipeline import _workspace
    cfg, W, pipe, lat, cp, cn, vc = tiny
    ctx = torch.cat([cp, cn])
    ld, cd, vd = lat.cuda(), ctx.cuda(), vc.cuda()

    def fwd():
        out = _product(pipe, ld, cd, vd, sliding_window_size=5, sliding_window_stride=3)
        torch.cuda.synchronize()
        return bits(out)
    first = fwd()
    ws = _workspace(ld.device)
    ptrs = {k: v.data_ptr() for k, v in ws.bufs.items()}
    mem = torch.cuda.memory_allocated()
    second = fwd()
    assert torch.equal(first, second)
    assert {k: v.data_ptr() for k, v in ws.bufs.items()} == ptrs
    assert torch.cuda.memory_allocated() == mem


# ------------------------------------------------------------------------------------------ pipeline
def _pipe_kw(cp, cn, vc):
    return dict(prompt_emb=cp, negative_prompt_emb=cn, vace_context=vc, seed=3, height=H, width=WD,
                num_frames=FRAMES, num_inference_steps=3, sliding_window_size=5, sliding_window_stride=3,
                output_type="latents")


def test_pipeline_euler_graph_equals_eager_equals_tiler(tiny):
    from vstyler import model_fn_wan_video
    from vstyler.options import host_options
    cfg, W, pipe, lat, cp, cn, vc = tiny
    kw = _pipe_kw(cp, cn, vc)
    graph = pipe(**kw)
    assert pipe.last_graph is not None
    assert graph.shape == (1, 16, T, H // 8, WD // 8)
    with host_options(graph=0):
        eager = pipe(**kw)
        assert pipe.last_graph is None
        pipe.model_fn = tiled_model_fn(model_fn_wan_video)
        try:
            tiled = pipe(**kw)
        finally:
            pipe.model_fn = model_fn_wan_video
    assert torch.equal(bits(graph), bits(eager))
    assert torch.equal(bits(eager), bits(tiled))
    plain = pipe(**dict(kw, sliding_window_size=None, sliding_window_stride=None))
    assert not torch.equal(plain, graph)


def test_pipeline_reference_frame_in_front(tiny):
    """One vace_reference_image latent frame in front: T + 1 = 10 frames, windows (0,5) (3,8) (6,10),
    no special-casing of the reference frame; the output drops it."""
    from vstyler.options import host_options
    cfg, W, pipe, lat, cp, cn, vc = tiny
    vc10 = O.synthetic_inputs(cfg, FRAMES + 4, H, WD)[3]
    assert vc10.shape[2] == T + 1
    kw = dict(_pipe_kw(cp, cn, vc10), vace_reference_image=torch.zeros(H, WD, 3, dtype=torch.uint8))
    graph = pipe(**kw)
    assert pipe.last_graph is not None
    assert graph.shape == (1, 16, T, H // 8, WD // 8)
    with host_options(graph=0):
        eager = pipe(**kw)
    assert torch.equal(bits(graph), bits(eager))


def test_denoise_unipc_windowed_equals_tiler(tiny):
    from vstyler import model_fn_wan_video
    cfg, W, pipe, lat, cp, cn, vc = tiny
    kw = dict(num_inference_steps=2, vace_scale=0.975, cfg_scale=1.2, sigma_shift=2.0, slg_blocks=(2,),
              slg_range=(0.0, 1.0), sliding_window_size=5, sliding_window_stride=3)
    got = pipe.denoise_unipc(lat, cp.cuda(), cn.cuda(), vc.cuda(), **kw)
    pipe.model_fn = tiled_model_fn(model_fn_wan_video)
    try:
        want = pipe.denoise_unipc(lat, cp.cuda(), cn.cuda(), vc.cuda(), **kw)
    finally:
        pipe.model_fn = model_fn_wan_video
    assert got.shape == lat.shape and torch.equal(bits(got), bits(want))
    assert not torch.equal(got, pipe.denoise_unipc(lat, cp.cuda(), cn.cuda(), vc.cuda(),
                                                   **dict(kw, sliding_window_size=None)))


def test_window_errors(tiny):
    cfg, W, pipe, lat, cp, cn, vc = tiny
    kw = dict(_pipe_kw(cp, cn, vc))
    for size, stride in ((5, None), (3, 5), (5, 0), (5.0, 3), (5, "3")):
        with pytest.raises(ValueError, match="sliding_window"):
            pipe(**dict(kw, sliding_window_size=size, sliding_window_stride=stride))
        with pytest.raises(ValueError, match="sliding_window"):
            _product(pipe, lat, cp, vc, sliding_window_size=size, sliding_window_stride=stride)
        with pytest.raises(ValueError, match="sliding_window"):
            pipe.denoise_unipc(lat, cp.cuda(), cn.cuda(), vc.cuda(), sliding_window_size=size,
                               sliding_window_stride=stride)
    with pytest.raises(NotImplementedError, match="tea_cache"):
        pipe(tea_cache_l1_thresh=0.05, tea_cache_model_id="Wan2.1-T2V-1.3B", **kw)


# ------------------------------------------------------------------------------------------ Ulysses
def _sp_worker(rank, world, port, q):
    try:
        _init(rank, world, port)
        from sp_util import HostStagedUlysses
        from vstyler import kernels as K
        from vstyler import model_fn_wan_video
        cfg = O.WAN_CONFIGS["tiny"]
        W = O.random_weights(cfg, seed=5)
        dit, vace = build(cfg, W, "cuda:0")
        lat, cp, cn, vc = O.synthetic_inputs(cfg, FRAMES, H, WD)
        t = _timestep().cuda()
        ctx = torch.cat([cp, cn]).cuda()

        def fwd(sp):
            out = model_fn_wan_video(dit, vace=vace, latents=lat.cuda(), timestep=t, context=ctx,
                                     vace_context=vc.cuda(), use_unified_sequence_parallel=sp is not None,
                                     sp_group=sp, sliding_window_size=5, sliding_window_stride=3)
            torch.cuda.synchronize()
            return out.cpu()
        with K.options(gemm_split=0, attn_split=0):
            single = fwd(None)
            sp = HostStagedUlysses()
            par = fwd(sp)
        q.put((rank, {"same": torch.equal(single, par), "calls": sp.collective_calls}))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))


def test_windowed_forward_under_ulysses_equals_sp1():
    """World 2, host-staged collectives on one GPU: windows of 5, 5 and 3 frames of 24 tokens (60 / 36
    tokens per rank); with split tails off the sharded windowed forward is bit-identical to SP = 1."""
    res = _spawn(_sp_worker, 2, timeout=300)
    assert len(res) == 2
    for rank, r in res:
        assert isinstance(r, dict), res
        assert r["same"] is True, (rank, r)
        assert r["calls"] > 0, (rank, r)
