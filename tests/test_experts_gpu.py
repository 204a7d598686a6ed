"""Two-expert denoising on the GPU (dit2 / vace2, the Wan2.2 A14B layout) and the enhancer pass.

vs_resize_nearest_u8 bit-exact against torch's nearest interpolate; the Euler and UniPC loops with two
experts bit-exact against test-side loops that call model_fn_wan_video with the expert the boundary
selects (eager, hipGraph, windows, V2V, fp8 + hot-loaded LoRA, Ulysses) and within the oracle's floor
of the oracle chain; the loader's file order; WanVideoPipeline.enhance against its steps done by hand.

Tiny config (dim 256, 2 heads, 4 layers, VACE at 0 and 2); expert 1 = random_weights(seed 5), expert 2 =
seed 6; T = 5 latent frames of 64x96.  Euler 4 steps shift 5: 1000, 937.5, 833.33, 625 (boundary 0.875:
2 | 2).  UniPC 6 steps shift 2: 999, 908, 799, 666, 499, 285 (2 | 4)."""
import pytest
import torch
import torch.nn.functional as F

from gpu_util import err
from oracle import wan_oracle as O
from oracle import wan_vae_oracle as V
from test_model_gpu import build
from test_sp import _init, _spawn
from vae_util import TINY_VAE

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
H, WD, FR = 64, 96, 17          # 17 frames -> T = 5 latent frames
TS, ST = (4, 6), (2, 3)


def bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


# ------------------------------------------------------------------------------------------ kernel
def _frames(t, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (t, h, w, 3), generator=g, dtype=torch.uint8)


def _torch_nearest(frames, ho, wo):
    x = frames.permute(0, 3, 1, 2).float()
    return F.interpolate(x, size=(ho, wo), mode="nearest").to(torch.uint8).permute(0, 2, 3, 1).contiguous()


RESIZES = [((6, 10), (9, 16)), ((16, 24), (6, 10)), ((7, 13), (7, 13)), ((1, 1), (3, 5)), ((5, 11), (8, 17))]


@pytest.mark.parametrize("src_hw,dst_hw", RESIZES)
def test_resize_nearest_u8_bit_exact(src_hw, dst_hw):
    """2 frames.  Output bytes 864 and 816 (whole 16-byte chunks), 360, 546 and 90 (element tails); a row
    of 8x17 is 51 bytes, so rows start at every alignment.  Then the same into a destination 1 and 5 bytes
    off a 16-byte boundary (element head), with the bytes around it untouched."""
    from vstyler import kernels as K
    src = _frames(2, *src_hw, seed=sum(src_hw))
    want = _torch_nearest(src, *dst_hw)
    sd = src.cuda()
    got = K.resize_nearest_u8(sd, *dst_hw)
    assert got.dtype == torch.uint8 and got.shape == (2, *dst_hw, 3)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(sd.cpu(), src), "the source was written"
    n = want.numel()
    for off in (1, 5):
        buf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        out = buf[16 + off:16 + off + n].view(2, *dst_hw, 3)
        assert K.resize_nearest_u8(sd, *dst_hw, out=out) is out
        assert torch.equal(out.cpu(), want), off
        assert (buf[:16 + off] == 0xA5).all() and (buf[16 + off + n:] == 0xA5).all(), off


def test_resize_nearest_u8_invalid_arguments():
    from vstyler import _lib, kernels as K
    lib = _lib.load()
    f = 1 << 20             # never dereferenced: validation fails first
    assert lib.vs_resize_nearest_u8(None, f, 2, 6, 10, 9, 16, 3, None) == 1
    assert lib.vs_resize_nearest_u8(f, None, 2, 6, 10, 9, 16, 3, None) == 1
    for sizes in ((0, 6, 10, 9, 16), (2, 0, 10, 9, 16), (2, 6, 0, 9, 16), (2, 6, 10, 0, 16), (2, 6, 10, 9, 0),
                  (2, 6, 10, 9, -1)):
        assert lib.vs_resize_nearest_u8(f, f + 4096, *sizes, 3, None) == 1, sizes
    assert lib.vs_resize_nearest_u8(f, f + 4096, 2, 6, 10, 9, 16, 4, None) == 1
    assert lib.vs_resize_nearest_u8(f, f + 4096, 2, 6, 10, 9, 16, 1, None) == 1
    x = torch.zeros((2, 6, 10, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        K.resize_nearest_u8(x.float(), 9, 16)
    with pytest.raises(ValueError):
        K.resize_nearest_u8(x[:, :, ::2], 9, 16)
    with pytest.raises(ValueError):
        K.resize_nearest_u8(x, 9, 16, out=torch.zeros((2, 9, 15, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="VS_E_INVALID"):
        K.resize_nearest_u8(torch.zeros((2, 6, 10, 4), dtype=torch.uint8, device="cuda"), 9, 16)


# ------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def two():
    from vstyler import WanVideoPipeline
    cfg = O.WAN_CONFIGS["tiny"]
    W1, W2 = O.random_weights(cfg, seed=5), O.random_weights(cfg, seed=6)
    pipe = WanVideoPipeline(device="cuda")
    pipe.dit, pipe.vace = build(cfg, W1)
    pipe.dit2, pipe.vace2 = build(cfg, W2)
    lat, cp, cn, vc = O.synthetic_inputs(cfg, FR, H, WD)
    assert lat.shape[2] == 5
    return cfg, W1, W2, pipe, lat, cp, cn, vc


class single:
    """The pipeline with one expert only (`which` = 1 or 2, as pipe.dit / pipe.vace) for a with-block."""

    def __init__(self, pipe, which):
        self.pipe, self.which = pipe, which

    def __enter__(self):
        p = self.pipe
        self.saved = (p.dit, p.vace, p.dit2, p.vace2)
        if self.which == 2:
            p.dit, p.vace = p.dit2, p.vace2
        p.dit2 = p.vace2 = None
        return p

    def __exit__(self, *exc):
        p = self.pipe
        p.dit, p.vace, p.dit2, p.vace2 = self.saved


class counting:
    """Records which expert every model_fn call of an eager loop runs on."""

    def __init__(self, pipe):
        self.pipe, self.calls = pipe, []

    def __enter__(self):
        from vstyler import model_fn_wan_video
        names = {id(self.pipe.dit): 1, id(self.pipe.dit2): 2}
        vaces = {1: self.pipe.vace, 2: self.pipe.vace2}

        def fn(dit=None, vace=None, **kw):
            e = names[id(dit)]
            assert vace is vaces[e]
            self.calls.append(e)
            return model_fn_wan_video(dit=dit, vace=vace, **kw)
        self.pipe.model_fn = fn
        return self.calls

    def __exit__(self, *exc):
        from vstyler import model_fn_wan_video
        self.pipe.model_fn = model_fn_wan_video


def euler_loop(pipe, start, cp, cn, vc, steps=4, boundary=0.875, scales=(5.0, 5.0), strength=1.0, **fwd):
    """The test-side loop: per step, model_fn_wan_video on the expert the boundary selects (expert 2 iff
    the fp32 timestep is below boundary * 1000), then vs_cfg_euler_dev.  scales: (expert 1, expert 2)."""
    from vstyler import kernels as K
    from vstyler import model_fn_wan_video
    from vstyler.flow_match import FlowMatchScheduler
    sch = FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
    sch.set_timesteps(steps, denoising_strength=strength, shift=5.0)
    experts = {1: (pipe.dit, pipe.vace), 2: (pipe.dit2, pipe.vace2)}
    lat = start.cuda().to(BF16).contiguous().clone()
    both = torch.cat([cp, cn]).cuda()
    for i, t in enumerate(sch.timesteps):
        e = 2 if float(t) < boundary * 1000 else 1
        dit, vace = experts[e]
        cfg_on = scales[e - 1] != 1.0
        v = model_fn_wan_video(dit, vace=vace, latents=lat, timestep=t.reshape(1).to(BF16).cuda(),
                               context=both if cfg_on else cp.cuda(), vace_context=None if vc is None else vc.cuda(),
                               **fwd)
        d = torch.tensor([sch.delta(i)], dtype=torch.float32, device="cuda")
        K.cfg_euler_dev(v[0:1], v[1:2] if cfg_on else None, lat, scales[e - 1], d)
    return lat


def _denoise(pipe, lat, cp, cn, vc, **kw):
    return pipe.denoise(lat, cp.cuda(), cn.cuda(), None if vc is None else vc.cuda(), **kw)


# ------------------------------------------------------------------------------------------ Euler
def test_euler_two_experts_equals_the_test_side_loop(two):
    from vstyler.pipeline import _workspace
    cfg, W1, W2, pipe, lat, cp, cn, vc = two
    want = euler_loop(pipe, lat, cp, cn, vc)
    eager = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4, use_graph=False)
    assert pipe.last_graph is None and pipe.last_graphs == [None, None]
    # equal-shaped experts share every Workspace buffer: a second run allocates and moves nothing
    torch.cuda.synchronize()
    ws = _workspace(torch.device("cuda", torch.cuda.current_device()))
    ptrs = {k: v.data_ptr() for k, v in ws.bufs.items()}
    again = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4, use_graph=False)
    torch.cuda.synchronize()
    assert {k: v.data_ptr() for k, v in ws.bufs.items()} == ptrs
    assert torch.equal(bits(again), bits(eager))
    with single(pipe, 1):
        _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4, use_graph=False)
    assert {k: v.data_ptr() for k, v in ws.bufs.items()} == ptrs, "one expert's buffers differ from the pair's"
    graph = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4, use_graph=True)
    assert len(pipe.last_graphs) == 2 and all(g is not None for g in pipe.last_graphs)
    assert pipe.last_graph is pipe.last_graphs[-1]
    assert torch.equal(bits(eager), bits(want))
    assert torch.equal(bits(graph), bits(want))
    assert {k: v.data_ptr() for k, v in ws.bufs.items()} == ptrs


def test_euler_two_experts_differs_from_both_single_expert_runs(two):
    """Fails where dit2 is ignored: the run would equal expert 1's."""
    cfg, W1, W2, pipe, lat, cp, cn, vc = two
    both = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4)
    with single(pipe, 1):
        one = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4)
        assert pipe.last_graphs == [pipe.last_graph] and pipe.last_graph is not None
        eager = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4, use_graph=False)
        assert torch.equal(bits(one), bits(eager))          # the single-expert capture, as before
    with single(pipe, 2):
        other = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4)
    assert not torch.equal(both, one) and not torch.equal(both, other) and not torch.equal(one, other)
    e1, e2 = err(both, one)[1], err(both, other)[1]
    print(f"two experts vs expert 1 alone: rel-L2 {e1:.4g}; vs expert 2 alone: {e2:.4g}")
    assert e1 > 1e-2 and e2 > 1e-2


def test_euler_two_experts_vs_oracle_chain(two):
    cfg, W1, W2, pipe, lat, cp, cn, vc = two
    got = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4)

    def chain():
        sigmas, timesteps = O.set_timesteps(4, 1.0, 5.0)
        x = lat
        for i, ts in enumerate(timesteps):
            W = W2 if float(ts) < 875.0 else W1
            t = ts.unsqueeze(0).to(BF16)
            vp = O.model_fn(W, cfg, x, t, cp, vc)
            vn = O.model_fn(W, cfg, x, t, cn, vc)
            x = O.cfg_euler(vp, vn, x, 5.0, O.euler_delta(sigmas, i))
        return x
    ref = chain()
    old = O.ACC_DTYPE
    O.ACC_DTYPE = torch.float64
    try:
        ref64 = chain()
    finally:
        O.ACC_DTYPE = old
    fmx, frel = err(ref64, ref)
    mx, rel = err(got, ref)
    print(f"euler two experts: max-abs {mx:.4g} rel-L2 {rel:.4g} (floor {fmx:.4g} / {frel:.4g})")
    assert rel <= 1.5 * frel + 2e-3 and mx <= 1.5 * fmx + 2e-2


def test_same_weights_twice_equal_the_single_expert_run(two):
    cfg, W1, W2, pipe, lat, cp, cn, vc = two
    with single(pipe, 1):
        want = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4)
    saved = (pipe.dit2, pipe.vace2)
    pipe.dit2, pipe.vace2 = build(cfg, W1)
    try:
        got = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4)
        assert len(pipe.last_graphs) == 2
        eager = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4, use_graph=False)
    finally:
        pipe.dit2, pipe.vace2 = saved
    assert torch.equal(bits(got), bits(want)) and torch.equal(bits(eager), bits(want))


@pytest.mark.parametrize("boundary,calls", [(0.875, [1, 1, 2, 2]), (0.9375, [1, 1, 2, 2]), (1.0, [1, 2, 2, 2]),
                                            (0, [1, 1, 1, 1]), (1.001, [2, 2, 2, 2]), (0.7, [1, 1, 1, 2])])
def test_euler_boundary_edges(two, boundary, calls):
    """937.5 is not strictly below 0.9375 * 1000, 1000 not below 1000; a boundary of 0 never switches,
    1.001 hands every step to expert 2."""
    cfg, W1, W2, pipe, lat, cp, cn, vc = two
    with counting(pipe) as seen:
        got = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4, use_graph=False, switch_DiT_boundary=boundary)
    assert seen == calls
    assert len(pipe.last_graphs) == len(set(calls))
    assert torch.equal(bits(got), bits(euler_loop(pipe, lat, cp, cn, vc, boundary=boundary)))


def test_single_expert_ignores_the_boundary(two):
    cfg, W1, W2, pipe, lat, cp, cn, vc = two
    with single(pipe, 1):
        want = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4)
        for b in (0, 1.001):
            assert torch.equal(bits(_denoise(pipe, lat, cp, cn, vc, num_inference_steps=4, switch_DiT_boundary=b)),
                               bits(want))
            assert len(pipe.last_graphs) == 1
        with pytest.raises(ValueError, match="second expert"):
            _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4, cfg_scale=(3.0, 5.0))
        with pytest.raises(ValueError, match="second expert"):
            pipe.denoise_unipc(lat, cp.cuda(), cn.cuda(), vc.cuda(), num_inference_steps=6, cfg_scale=(1.2, 2.0))


def test_euler_cfg_scale_pair(two):
    """(low_noise, high_noise) = (3.0, 5.0): 5.0 before the switch, 3.0 after; a scale of exactly 1.0 runs
    the batch-1 forward on that expert."""
    cfg, W1, W2, pipe, lat, cp, cn, vc = two
    got = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4, cfg_scale=(3.0, 5.0))
    assert torch.equal(bits(got), bits(euler_loop(pipe, lat, cp, cn, vc, scales=(5.0, 3.0))))
    assert not torch.equal(got, euler_loop(pipe, lat, cp, cn, vc, scales=(3.0, 5.0)))
    batches = []
    from vstyler import model_fn_wan_video

    def fn(**kw):
        batches.append(kw["context"].shape[0])
        return model_fn_wan_video(**kw)
    pipe.model_fn = fn
    try:
        one = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4, cfg_scale=(1.0, 5.0), use_graph=False)
    finally:
        pipe.model_fn = model_fn_wan_video
    assert batches == [2, 2, 1, 1]
    assert torch.equal(bits(one), bits(euler_loop(pipe, lat, cp, cn, vc, scales=(5.0, 1.0))))
    for bad in ((3.0,), (1.0, 2.0, 3.0), "5", (3.0, None)):
        with pytest.raises(ValueError, match="cfg_scale"):
            _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4, cfg_scale=bad)


def test_euler_two_experts_with_sliding_windows(two):
    """Windows (5, 2) over T = 9: every segment's capture holds all windows of its expert's step."""
    cfg, W1, W2, pipe, _, cp, cn, _ = two
    lat, _, _, vc = O.synthetic_inputs(cfg, 33, H, WD)
    assert lat.shape[2] == 9
    kw = dict(sliding_window_size=5, sliding_window_stride=2)
    got = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4, **kw)
    assert len(pipe.last_graphs) == 2 and all(g is not None for g in pipe.last_graphs)
    assert torch.equal(bits(got), bits(euler_loop(pipe, lat, cp, cn, vc, **kw)))
    assert not torch.equal(got, _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4))


def test_euler_v2v_two_experts(two):
    """Strength 0.6, 3 steps: 882, 769, 556; boundary 0.8 splits them 1 | 2 (a one-step first segment
    runs eager, the second is captured)."""
    cfg, W1, W2, pipe, x0, cp, cn, vc = two
    kw = dict(prompt_emb=cp, negative_prompt_emb=cn, vace_context=vc, seed=3, height=H, width=WD, num_frames=FR,
              num_inference_steps=3, denoising_strength=0.6, switch_DiT_boundary=0.8, output_type="latents")
    got = pipe(input_latents=x0, **kw)
    assert [g is not None for g in pipe.last_graphs] == [False, True]
    from vstyler.flow_match import FlowMatchScheduler
    sch = FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
    sch.set_timesteps(3, denoising_strength=0.6, shift=5.0)
    assert [round(float(t)) for t in sch.timesteps] == [882, 769, 556]
    noise = O.generate_noise(tuple(x0.shape), 3)
    start = sch.add_noise(x0.cuda(), noise.cuda(), sch.timesteps[0])
    want = euler_loop(pipe, start, cp, cn, vc, steps=3, boundary=0.8, strength=0.6)
    assert torch.equal(bits(got), bits(want))
    with counting(pipe) as seen:
        from vstyler.options import host_options
        with host_options(graph=0):
            eager = pipe(input_latents=x0, **kw)
    assert seen == [1, 2, 2] and torch.equal(bits(eager), bits(want))


def test_vace2_missing_runs_expert_two_without_hints(two):
    cfg, W1, W2, pipe, lat, cp, cn, vc = two
    saved, pipe.vace2 = pipe.vace2, None
    try:
        got = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4)
        want = euler_loop(pipe, lat, cp, cn, vc)
    finally:
        pipe.vace2 = saved
    assert torch.equal(bits(got), bits(want))
    assert not torch.equal(got, _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4))


def test_tea_cache_with_a_second_expert_raises(two):
    cfg, W1, W2, pipe, lat, cp, cn, vc = two
    with pytest.raises(NotImplementedError, match="second expert"):
        pipe(prompt_emb=cp, negative_prompt_emb=cn, vace_context=vc, seed=3, height=H, width=WD, num_frames=FR,
             num_inference_steps=4, tea_cache_l1_thresh=0.05, tea_cache_model_id="Wan2.1-T2V-1.3B",
             output_type="latents")
    from vstyler.teacache import TeaCache
    with pytest.raises(NotImplementedError, match="second expert"):
        _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4,
                 tea_cache=TeaCache(4, rel_l1_thresh=0.05, model_id="Wan2.1-T2V-1.3B"))


# ------------------------------------------------------------------------------------------ UniPC
def unipc_loop(pipe, noise, cp, cn, vc, n=6, boundary=0.875, scales=(1.2, 1.2), slg_blocks=(), slg_range=(0.2, 0.7),
               vace_scale=1.0, x0=None, fwd=None, back=None):
    """denoise_unipc's step restated around the expert the boundary selects (int64 timestep below
    boundary * 1000 -> expert 2)."""
    from vstyler import kernels as K
    from vstyler import model_fn_wan_video
    from vstyler.unipc import FlowUniPCMultistepScheduler, cast
    sched = FlowUniPCMultistepScheduler(shift=1.0)
    sched.set_timesteps(n, shift=2.0)
    experts = {1: (pipe.dit, pipe.vace), 2: (pipe.dit2, pipe.vace2)}
    x = noise.cuda().float().contiguous().clone()
    first = 0
    if x0 is not None:
        x = sched.add_noise(x0.cuda().float().contiguous(), x, sched.timesteps[n - fwd])
        first = n - back
    both = torch.cat([cp, cn]).cuda()
    for i in range(first, n):
        t = sched.timesteps[i]
        e = 2 if int(t) < boundary * 1000 else 1
        dit, vace = experts[e]
        cfg_on = scales[e - 1] != 1.0
        lat16 = cast(x, torch.empty(x.shape, dtype=BF16, device="cuda"))
        slg = tuple(slg_blocks) if slg_range[0] <= i / n <= slg_range[1] else ()
        v = model_fn_wan_video(dit, vace=vace, latents=lat16, timestep=t.reshape(1).to(dtype=BF16, device="cuda"),
                               context=both if cfg_on else cp.cuda(), vace_context=vc.cuda(), vace_scale=vace_scale,
                               slg_blocks=slg)
        v16 = torch.zeros(x.shape, dtype=BF16, device="cuda")
        K.cfg_euler(v[0:1], v[1:2] if cfg_on else None, v16, scales[e - 1], 1.0)
        x = sched.step(cast(v16, torch.empty_like(x)), t, x)[0]
    return cast(x, torch.empty(x.shape, dtype=BF16, device="cuda"))


def test_unipc_two_experts_slg_and_pair(two):
    cfg, W1, W2, pipe, lat, cp, cn, vc = two
    kw = dict(num_inference_steps=6, sigma_shift=2.0, vace_scale=0.975, slg_blocks=(2,))
    with counting(pipe) as seen:
        got = pipe.denoise_unipc(lat, cp.cuda(), cn.cuda(), vc.cuda(), cfg_scale=(1.2, 2.0), **kw)
    assert seen == [1, 1, 2, 2, 2, 2]
    want = unipc_loop(pipe, lat, cp, cn, vc, scales=(2.0, 1.2), slg_blocks=(2,), vace_scale=0.975)
    assert torch.equal(bits(got), bits(want))
    with single(pipe, 1):
        one = pipe.denoise_unipc(lat, cp.cuda(), cn.cuda(), vc.cuda(), cfg_scale=2.0, **kw)
    assert not torch.equal(got, one)


def test_unipc_enhancer_pass_runs_on_dit2_alone(two):
    """f = 4, b = 3 of 6: re-noise at 799, steps 666, 499, 285, all below 875; pipe.dit is never touched."""
    cfg, W1, W2, pipe, x0, cp, cn, vc = two
    noise = O.generate_noise(tuple(x0.shape), 9)
    kw = dict(num_inference_steps=6, sigma_shift=2.0, input_latents=x0, forward_step=4, skip_backward_step=3)
    saved = (pipe.dit, pipe.vace)
    pipe.dit = pipe.vace = None
    try:
        got = pipe.denoise_unipc(noise, cp.cuda(), cn.cuda(), vc.cuda(), cfg_scale=(1.2, 2.0), **kw)
        with pytest.raises(RuntimeError, match="expert 1"):
            pipe.denoise_unipc(noise, cp.cuda(), cn.cuda(), vc.cuda(), cfg_scale=(1.2, 2.0),
                               switch_DiT_boundary=0.5, **kw)
    finally:
        pipe.dit, pipe.vace = saved
    with single(pipe, 2):
        want = pipe.denoise_unipc(noise, cp.cuda(), cn.cuda(), vc.cuda(), cfg_scale=1.2, **kw)
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(got), bits(unipc_loop(pipe, noise, cp, cn, vc, x0=x0, fwd=4, back=3)))
    # boundary 0.5: 666 on expert 1, 499 and 285 on expert 2
    with counting(pipe) as seen:
        half = pipe.denoise_unipc(noise, cp.cuda(), cn.cuda(), vc.cuda(), cfg_scale=1.2, switch_DiT_boundary=0.5,
                                  **kw)
    assert seen == [1, 2, 2]
    assert torch.equal(bits(half), bits(unipc_loop(pipe, noise, cp, cn, vc, boundary=0.5, x0=x0, fwd=4, back=3)))
    assert not torch.equal(half, got)


# ------------------------------------------------------------------------------------------ fp8 and LoRA
def test_fp8_experts_with_a_lora_hot_loaded_on_vace2(two):
    from test_fp8_lora_gpu import TARGETS
    from vstyler import WanVideoPipeline
    from vstyler.models import quantize_fp8_
    cfg, W1, W2, _, lat, cp, cn, vc = two
    pipe = WanVideoPipeline(device="cuda")
    pipe.dit, pipe.vace = build(cfg, W1)
    pipe.dit2, pipe.vace2 = build(cfg, W2)
    for m in (pipe.dit, pipe.vace, pipe.dit2, pipe.vace2):
        quantize_fp8_(m)
    plain = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4)
    g = torch.Generator().manual_seed(8)
    r, D, Fd = 32, cfg["dim"], cfg["ffn_dim"]
    lora = {}
    for i in range(len(cfg["vace_layers"])):
        for t in TARGETS:
            out_f, in_f = {"ffn.0": (Fd, D), "ffn.2": (D, Fd)}.get(t, (D, D))
            lora[f"vace_blocks.{i}.{t}.lora_A.default.weight"] = (0.05 * torch.randn(r, in_f, generator=g)).to(BF16)
            lora[f"vace_blocks.{i}.{t}.lora_B.default.weight"] = (0.05 * torch.randn(out_f, r, generator=g)).to(BF16)
    n = pipe.load_lora(pipe.vace2, alpha=2.0, hotload=True, state_dict={k: v.cuda() for k, v in lora.items()})
    assert n == len(TARGETS) * len(cfg["vace_layers"])
    graph = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4)
    assert len(pipe.last_graphs) == 2 and all(x is not None for x in pipe.last_graphs)
    eager = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4, use_graph=False)
    want = euler_loop(pipe, lat, cp, cn, vc)
    assert torch.equal(bits(graph), bits(want)) and torch.equal(bits(eager), bits(want))
    assert not torch.equal(graph, plain)                     # the adapter on expert 2's VACE moved the result
    # expert 1's steps do not see it: the first two steps of both runs agree
    head = _denoise(pipe, lat, cp, cn, vc, num_inference_steps=4, switch_DiT_boundary=0)
    with single(pipe, 1):
        assert torch.equal(bits(head), bits(_denoise(pipe, lat, cp, cn, vc, num_inference_steps=4)))


# ------------------------------------------------------------------------------------------ Ulysses
def _sp_worker(rank, world, port, q):
    try:
        _init(rank, world, port)
        from sp_util import HostStagedUlysses
        from vstyler import WanVideoPipeline
        from vstyler import kernels as K
        cfg = O.WAN_CONFIGS["tiny"]
        pipe = WanVideoPipeline(device="cuda:0")
        pipe.dit, pipe.vace = build(cfg, O.random_weights(cfg, seed=5), "cuda:0")
        pipe.dit2, pipe.vace2 = build(cfg, O.random_weights(cfg, seed=6), "cuda:0")
        lat, cp, cn, vc = O.synthetic_inputs(cfg, FR, H, WD)
        calls = []
        from vstyler import model_fn_wan_video

        def fn(dit=None, **kw):
            calls.append(1 if dit is pipe.dit else 2)
            return model_fn_wan_video(dit=dit, **kw)
        pipe.model_fn = fn
        with K.options(gemm_split=0, attn_split=0):
            single_ = pipe.denoise(lat, cp.cuda(), cn.cuda(), vc.cuda(), num_inference_steps=4, use_graph=False)
            torch.cuda.synchronize()
            sp = HostStagedUlysses()
            pipe.sp_group, pipe.use_unified_sequence_parallel = sp, True
            par = pipe.denoise(lat, cp.cuda(), cn.cuda(), vc.cuda(), num_inference_steps=4)
            torch.cuda.synchronize()
        q.put((rank, {"same": torch.equal(single_.cpu(), par.cpu()), "calls": sp.collective_calls,
                      "experts": calls, "graphs": pipe.last_graphs}))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))


def test_two_experts_under_ulysses_equal_sp1():
    """World 2, host-staged collectives on one GPU, split tails off: the sharded two-expert Euler loop is
    bit-identical to SP = 1 (host-staged collectives are not capturable: eager segments)."""
    res = _spawn(_sp_worker, 2, timeout=300)
    assert len(res) == 2
    for rank, r in res:
        assert isinstance(r, dict), res
        assert r["same"] is True, (rank, r)
        assert r["calls"] > 0, (rank, r)
        assert r["experts"] == [1, 1, 2, 2] * 2 and r["graphs"] == [None, None], (rank, r)


# ------------------------------------------------------------------------------------------ loader
def _save(path, W, vace):
    from safetensors.torch import save_file
    save_file({k: v.contiguous() for k, v in W.items() if vace or not k.startswith("vace")}, str(path))
    return str(path)


def _pretrained(paths, **kw):
    from vstyler import ModelConfig, WanVideoPipeline
    return WanVideoPipeline.from_pretrained(torch_dtype=BF16, device="cuda",
                                            model_configs=[ModelConfig(path=p) for p in paths], **kw)


def test_loader_two_experts_in_file_order(two, tmp_path):
    cfg, W1, W2 = two[:3]
    key, vkey = "blocks.1.ffn.0.weight", "vace_blocks.1.ffn.2.weight"
    assert not torch.equal(W1[key], W2[key])
    hi, lo = _save(tmp_path / "high_noise.safetensors", W1, False), _save(tmp_path / "low_noise.safetensors", W2, False)
    pipe = _pretrained([hi, lo])
    assert torch.equal(pipe.dit.state_dict()[key].cpu(), W1[key])
    assert torch.equal(pipe.dit2.state_dict()[key].cpu(), W2[key])
    assert pipe.vace is None and pipe.vace2 is None
    pipe = _pretrained([lo, hi])
    assert torch.equal(pipe.dit.state_dict()[key].cpu(), W2[key])
    assert torch.equal(pipe.dit2.state_dict()[key].cpu(), W1[key])
    # one file loads as before
    pipe = _pretrained([hi])
    assert torch.equal(pipe.dit.state_dict()[key].cpu(), W1[key]) and pipe.dit2 is None and pipe.vace2 is None
    # combined DiT + VACE files: one of each per file
    c1, c2 = _save(tmp_path / "c1.safetensors", W1, True), _save(tmp_path / "c2.safetensors", W2, True)
    pipe = _pretrained([c1, c2])
    assert torch.equal(pipe.dit2.state_dict()[key].cpu(), W2[key])
    assert torch.equal(pipe.vace.state_dict()[vkey].cpu(), W1[vkey])
    assert torch.equal(pipe.vace2.state_dict()[vkey].cpu(), W2[vkey])
    assert pipe.vace2.vace_layers == tuple(cfg["vace_layers"])
    # VACE-module-only files pair with the DiTs in order
    from safetensors.torch import save_file
    vs = []
    for name, W in (("v1", W1), ("v2", W2)):
        vs.append(str(tmp_path / f"{name}.safetensors"))
        save_file({k: v.contiguous() for k, v in W.items() if k.startswith("vace")}, vs[-1])
    pipe = _pretrained([hi, vs[0], lo, vs[1]])
    assert torch.equal(pipe.vace.state_dict()[vkey].cpu(), W1[vkey])
    assert torch.equal(pipe.vace2.state_dict()[vkey].cpu(), W2[vkey])
    assert torch.equal(pipe.dit2.state_dict()[key].cpu(), W2[key])
    with pytest.raises(ValueError, match="third DiT"):
        _pretrained([hi, lo, hi])
    with pytest.raises(ValueError, match="third VACE"):
        _pretrained([c1, c2, vs[0]])
    small = dict(cfg, dim=128, num_heads=1, ffn_dim=256)
    other = _save(tmp_path / "other_dim.safetensors", O.random_weights(small, seed=7), False)
    with pytest.raises(ValueError, match="differ in dim"):
        _pretrained([hi, other])
    fewer = _save(tmp_path / "fewer.safetensors", O.random_weights(dict(cfg, num_layers=2), seed=7, vace=False), False)
    with pytest.raises(ValueError, match="differ in num_layers"):
        _pretrained([hi, fewer])


def test_loader_keeps_each_experts_own_fp8_tensors(two, tmp_path):
    """fp8_weights="keep": every expert's block Linears run the e4m3 bytes of its own file."""
    from safetensors.torch import save_file
    cfg, W1, W2 = two[:3]
    paths = []
    for name, W in (("a", W1), ("b", W2)):
        sd = {}
        for k, v in W.items():
            if k.startswith("vace"):
                continue
            fp8 = k.startswith("blocks.") and k.endswith(".weight") and v.dim() == 2 and "norm" not in k
            sd[k] = v.to(torch.float8_e4m3fn) if fp8 else v.contiguous()
        paths.append(str(tmp_path / f"{name}_fp8.safetensors"))
        save_file(sd, paths[-1])
    pipe = _pretrained(paths, fp8_weights="keep")
    from vstyler.models import block_fp8_linears
    for dit, W in ((pipe.dit, W1), (pipe.dit2, W2)):
        ffn_up = block_fp8_linears(dit.blocks[1])[8]                  # loader._BLOCK_LINEARS: "ffn.0"
        w8 = W["blocks.1.ffn.0.weight"].to(torch.float8_e4m3fn).view(torch.uint8)
        assert torch.equal(ffn_up.weight_fp8.cpu(), w8)
    assert not torch.equal(block_fp8_linears(pipe.dit.blocks[1])[8].weight_fp8,
                           block_fp8_linears(pipe.dit2.blocks[1])[8].weight_fp8)


# ------------------------------------------------------------------------------------------ enhance
def test_enhance_equals_its_steps_by_hand(two):
    """5 frames of 32x48 -> 64x96, tiny VAE, 6 UniPC steps, f = 4, b = 3, the default guidance pair and
    boundary: only dit2 runs."""
    from vstyler import kernels as K
    from vstyler import vae
    from vstyler.vae import preprocess_video, vae_output_to_u8
    cfg, W1, W2, pipe, _, cp, cn, _ = two
    Wv = V.random_vae_weights(TINY_VAE, seed=34)
    pipe.vae = vae.WanVideoVAE(z_dim=16, dim=TINY_VAE["dim"], device="cuda").load_state_dict(Wv)
    video = _frames(5, 32, 48, 21)
    kw = dict(height=H, width=WD, num_inference_steps=6, sigma_shift=2.0, forward_step=4, skip_backward_step=3,
              seed=11, tile_size=TS, tile_stride=ST, prompt_emb=cp, negative_prompt_emb=cn)
    try:
        with counting(pipe) as seen:
            got = pipe.enhance(list(video.numpy()), output_type="u8", **kw)
        assert seen == [2, 2, 2]
        assert got.dtype == torch.uint8 and got.shape == (5, H, WD, 3)
        lat = pipe.enhance(video, output_type="latents", **kw)
        assert lat.shape == (1, 16, 2, H // 8, WD // 8) and lat.dtype == BF16
        # by hand, the resize by torch
        big = _torch_nearest(video, H, WD).cuda()
        assert torch.equal(K.resize_nearest_u8(video.cuda(), H, WD), big)
        x0 = pipe.vae.encode(preprocess_video(big), "cuda", tiled=True, tile_size=TS, tile_stride=ST)
        noise = pipe.generate_noise(tuple(x0.shape), seed=11)
        want = pipe.denoise_unipc(noise, cp.cuda(), cn.cuda(), cfg_scale=(3.0, 4.0), num_inference_steps=6,
                                  sigma_shift=2.0, input_latents=x0, forward_step=4, skip_backward_step=3)
        assert torch.equal(bits(lat), bits(want))
        dec = pipe.vae.decode(want, device="cuda", tiled=True, tile_size=TS, tile_stride=ST)
        assert torch.equal(got.cpu(), vae_output_to_u8(dec[0]).cpu())
        assert not torch.equal(got.cpu(), big.cpu())
        # frames already at the target size skip the resize
        same = pipe.enhance(big, output_type="latents", **kw)
        assert torch.equal(bits(same), bits(want))
        frames = pipe.enhance(video, **dict(kw, skip_backward_step=1))
        assert len(frames) == 5 and frames[0].size == (WD, H)
        with pytest.raises(ValueError, match=r"4k \+ 1"):
            pipe.enhance(_frames(6, 32, 48, 21), output_type="latents", **kw)
        with pytest.raises(ValueError, match="cfg_scale"):
            pipe.enhance(video, output_type="latents", cfg_scale=(3.0, 4.0, 5.0), **kw)
    finally:
        pipe.vae = None
