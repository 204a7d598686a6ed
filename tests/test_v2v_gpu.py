"""GPU parity of the video-to-video path: vs_flow_add_noise (bit-exact in both modes), the two
schedulers' add_noise, WanVideoPipeline.__call__(input_video= / input_latents=, denoising_strength=)
against the oracle chain restated for a shortened schedule (oracle.denoise fixes strength 1.0), and
denoise_unipc(input_latents=, forward_step=, skip_backward_step=), the enhancer's pass
(denoising_enhancing/wan/text2video.py:347-375)."""
import pytest
import torch

from gpu_util import err
from oracle import wan_oracle as O
from oracle import wan_vae_oracle as V
from oracle.unipc_oracle import UniPCOracle
from test_model_gpu import build
from vae_util import TINY_VAE

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
TS, ST = (4, 6), (2, 3)
H, WD = 64, 96


def bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def add_noise_bf16_ref(x0, noise, sigma):
    """flow_match.py:99 on bf16 tensors with a 0-d fp32 sigma, as torch evaluates it on a GPU: the
    sigma and 1 - sigma stay fp32, each product is one fp32 multiply rounded to bf16, the sum one
    fp32 add rounded to bf16.  (Torch on the CPU would first round the 0-d sigma to bf16.)"""
    s = torch.as_tensor(sigma, dtype=torch.float32)
    a = 1 - s
    p = (a * x0.float()).to(BF16)
    q = (s * noise.float()).to(BF16)
    return (p.float() + q.float()).to(BF16)


def v2v_sigma0():
    return O.set_timesteps(3, 0.6, 5.0)[0][0].item()


def _rand_bf16(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g).to(BF16)
    x[0::5] = 0.0
    x[2::7] = -0.0
    return x


# ------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("n", [8, 2056, 2880, 3072])
def test_flow_add_noise_bf16_bit_exact(n):
    """n = 8: one vector; 2056 = 257 vectors: a second block with one live thread; 2880 = 360
    vectors: a partly filled second block; 3072 (these tests' T = 5 latents): whole blocks only."""
    from vstyler import kernels as K
    x, z = _rand_bf16(n, 1), _rand_bf16(n, 2).roll(1)
    for sigma in (0.0, 1.0, 2.0 ** -10, torch.tensor(0.3, dtype=torch.float32).item(), v2v_sigma0()):
        ref = bits(add_noise_bf16_ref(x, z, sigma))
        xd, zd = x.cuda(), z.cuda()
        out = torch.full((n,), 7.0, dtype=BF16, device="cuda")
        assert K.flow_add_noise(xd, zd, sigma, out=out) is out
        assert torch.equal(bits(out), ref), (n, sigma)
        assert torch.equal(bits(xd), bits(x)) and torch.equal(bits(zd), bits(z))      # inputs untouched
        assert torch.equal(bits(K.flow_add_noise(xd, zd, sigma)), ref)                  # out allocated
        xa = x.cuda()
        K.flow_add_noise(xa, zd, sigma, out=xa)                                          # out aliases x0
        assert torch.equal(bits(xa), ref), (n, sigma, "alias x0")
        za = z.cuda()
        K.flow_add_noise(xd, za, sigma, out=za)                                          # out aliases noise
        assert torch.equal(bits(za), ref), (n, sigma, "alias noise")


@pytest.mark.parametrize("n", [1, 7, 1000, 3072])
def test_flow_add_noise_fp32_bit_exact(n):
    """(1 - s) * x + s * z op by op in fp32 (fm_solvers_unipc.py:797-799): a contraction of either
    product into the add changes low bits of most elements."""
    from vstyler import kernels as K
    g = torch.Generator().manual_seed(n)
    x, z = torch.randn(n, generator=g), torch.randn(n, generator=g)
    for sigma in (0.0, 1.0, 2.0 ** -10, 0.3, v2v_sigma0()):
        s = torch.tensor(sigma, dtype=torch.float32)
        a = 1 - s
        p = a * x
        q = s * z
        ref = bits(p + q)
        got = K.flow_add_noise(x.cuda(), z.cuda(), s.item())
        assert got.dtype == torch.float32 and torch.equal(bits(got), ref), (n, sigma)
        xa = x.cuda()
        K.flow_add_noise(xa, z.cuda(), s.item(), out=xa)
        assert torch.equal(bits(xa), ref)


def test_flow_match_add_noise_equals_torch_on_device():
    """FlowMatchScheduler.add_noise on bf16 device tensors == the reference expression evaluated by
    torch on the same device with the scheduler's 0-d fp32 CPU sigma (the authority for the bf16
    rounding contract), at every timestep of a shortened schedule."""
    from vstyler.flow_match import FlowMatchScheduler
    sch = FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
    sch.set_timesteps(3, denoising_strength=0.6, shift=5.0)
    x = _rand_bf16(16 * 2 * 8 * 12, 3).reshape(1, 16, 2, 8, 12).cuda()
    z = _rand_bf16(16 * 2 * 8 * 12, 4).roll(3).reshape(1, 16, 2, 8, 12).cuda()
    for i, t in enumerate(sch.timesteps):
        sigma = sch.sigmas[i]
        assert sigma.device.type == "cpu" and sigma.dim() == 0 and sigma.dtype == torch.float32
        want = (1 - sigma) * x + sigma * z
        got = sch.add_noise(x, z, t)
        assert got.dtype == BF16 and got.shape == x.shape
        assert torch.equal(bits(got), bits(want)), i
        assert torch.equal(bits(got), bits(add_noise_bf16_ref(x.cpu(), z.cpu(), sigma))), i
    # CPU tensors keep the torch expression
    xc, zc = x.cpu(), z.cpu()
    assert torch.equal(sch.add_noise(xc, zc, sch.timesteps[0]), (1 - sch.sigmas[0]) * xc + sch.sigmas[0] * zc)


def test_flow_add_noise_invalid_arguments():
    from vstyler import _lib, kernels as K
    lib = _lib.load()
    fake = 1 << 20          # aligned, never dereferenced: validation fails first
    assert lib.vs_flow_add_noise(None, fake, fake, 8, 0.5, 0, None) == 1
    assert lib.vs_flow_add_noise(fake, None, fake, 8, 0.5, 0, None) == 1
    assert lib.vs_flow_add_noise(fake, fake, None, 8, 0.5, 1, None) == 1
    assert lib.vs_flow_add_noise(fake, fake, fake, 0, 0.5, 0, None) == 1
    assert lib.vs_flow_add_noise(fake, fake, fake, 0, 0.5, 1, None) == 1
    assert lib.vs_flow_add_noise(fake, fake, fake, 12, 0.5, 0, None) == 1       # bf16: n % 8
    assert lib.vs_flow_add_noise(fake + 2, fake, fake, 8, 0.5, 0, None) == 1
    assert lib.vs_flow_add_noise(fake, fake, fake + 2, 8, 0.5, 0, None) == 1
    assert lib.vs_flow_add_noise(fake, fake + 2, fake, 8, 0.5, 1, None) == 1    # fp32: 4-byte alignment
    assert lib.vs_flow_add_noise(fake, fake, fake, 8, 0.5, 2, None) == 1
    assert lib.vs_flow_add_noise(fake, fake, fake, 8, 0.5, -1, None) == 1
    x = torch.zeros(16, dtype=BF16, device="cuda")
    with pytest.raises(ValueError):
        K.flow_add_noise(x, x.float(), 0.5)
    with pytest.raises(ValueError):
        K.flow_add_noise(x.to(torch.float16), x.to(torch.float16), 0.5)
    with pytest.raises(ValueError):
        K.flow_add_noise(x.reshape(4, 4).t(), x.reshape(4, 4).t(), 0.5)


# ------------------------------------------------------------------------------------------ pipeline
def _frames(t, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (t, h, w, 3), generator=g, dtype=torch.uint8)


def _vae_model(W):
    from vstyler import vae
    return vae.WanVideoVAE(z_dim=16, dim=TINY_VAE["dim"], device="cuda").load_state_dict(W)


@pytest.fixture(scope="module")
def tiny():
    from vstyler import WanVideoPipeline
    cfg = O.WAN_CONFIGS["tiny"]
    W = O.random_weights(cfg, seed=5)
    Wv = V.random_vae_weights(TINY_VAE, seed=34)
    pipe = WanVideoPipeline(device="cuda")
    pipe.dit, pipe.vace = build(cfg, W)
    pipe.vae = _vae_model(Wv)
    return cfg, W, Wv, pipe


def test_strength_one_is_the_identity(tiny):
    """sigma_0 of a strength-1 schedule is exactly 1, so the re-noised latents are the noise."""
    cfg, W, Wv, pipe = tiny
    T = 5
    x0, cp, cn, vc = O.synthetic_inputs(cfg, T, H, WD)
    kw = dict(prompt_emb=cp, negative_prompt_emb=cn, vace_context=vc, seed=3, height=H, width=WD, num_frames=T,
              num_inference_steps=2, output_type="latents")
    plain = pipe(**kw)
    got = pipe(input_latents=x0, denoising_strength=1.0, **kw)
    assert torch.equal(bits(got), bits(plain))
    assert not torch.equal(pipe(input_latents=x0, denoising_strength=0.6, **kw), plain)


def _euler_v2v_chain(cfg, W, Wv, video, vace_video, refimg, cp, cn, seed, strength, steps):
    """WanVideoPipeline.__call__ with input_video (wan_video_new.py:484, 578-614, 515-550) from the
    oracle's pieces."""
    t_lat = (video.shape[0] - 1) // 4 + 1
    x0 = V.tiled_encode(V.preprocess_video(video), Wv, TS, ST, TINY_VAE)
    vc, nref = None, 0
    rin = None if refimg is None else V.preprocess_video(refimg)
    if vace_video is not None:
        vc = V.vace_context(Wv, V.preprocess_video(vace_video), None, tiled=True, tile_size=TS, tile_stride=ST,
                            cfg=TINY_VAE, vace_reference_image=rin)
    if rin is not None:
        nref = 1
        x0 = torch.cat([V.vae_encode(rin, Wv, TINY_VAE), x0], dim=2)             # :608-609, untiled
    noise = O.generate_noise((1, 16, t_lat + nref, H // 8, WD // 8), seed)
    if nref:
        noise = torch.cat((noise[:, :, -nref:], noise[:, :, :-nref]), dim=2)
    sigmas, timesteps = O.set_timesteps(steps, strength, 5.0)
    lat = add_noise_bf16_ref(x0.to(BF16), noise, sigmas[0])                        # :613
    for i, ts in enumerate(timesteps):
        t = ts.unsqueeze(0).to(BF16)
        vp = O.model_fn(W, cfg, lat, t, cp, vc)
        vn = O.model_fn(W, cfg, lat, t, cn, vc)
        lat = O.cfg_euler(vp, vn, lat, 5.0, O.euler_delta(sigmas, i))
    return lat[:, :, nref:]


@pytest.mark.parametrize("case", ["video", "video+vace", "video+vace+ref"])
def test_euler_v2v_vs_oracle_chain(tiny, case):
    cfg, W, Wv, pipe = tiny
    T = 9 if case == "video+vace" else 5
    video = _frames(T, H, WD, 11)
    vace_video = _frames(T, H, WD, 12) if "vace" in case else None
    refimg = _frames(1, H, WD, 13) if "ref" in case else None
    _, cp, cn, _ = O.synthetic_inputs(cfg, T, H, WD)
    kw = {}
    if vace_video is not None:
        kw["vace_video"] = list(vace_video.numpy())
    if refimg is not None:
        kw["vace_reference_image"] = refimg[0].numpy()
    got = pipe(prompt_emb=cp, negative_prompt_emb=cn, input_video=list(video.numpy()), denoising_strength=0.6,
               seed=3, height=H, width=WD, num_frames=T, num_inference_steps=3, tile_size=TS, tile_stride=ST,
               output_type="latents", **kw)
    assert got.shape == (1, 16, (T - 1) // 4 + 1, H // 8, WD // 8)

    def chain():
        return _euler_v2v_chain(cfg, W, Wv, video, vace_video, refimg, cp, cn, 3, 0.6, 3)

    ref = chain()
    old = O.ACC_DTYPE
    O.ACC_DTYPE = torch.float64
    try:
        ref64 = chain()
    finally:
        O.ACC_DTYPE = old
    fmx, frel = err(ref64, ref)
    mx, rel = err(got, ref)
    print(f"euler v2v {case}: max-abs {mx:.4g} rel-L2 {rel:.4g} (floor {fmx:.4g} / {frel:.4g})")
    assert rel <= 1.5 * frel + 2e-3 and mx <= 1.5 * fmx + 2e-2


def test_input_video_validation(tiny):
    cfg, W, Wv, pipe = tiny
    T = 5
    video = _frames(T, H, WD, 11)
    x0, cp, cn, _ = O.synthetic_inputs(cfg, T, H, WD)
    kw = dict(prompt_emb=cp, negative_prompt_emb=cn, denoising_strength=0.6, seed=3, height=H, width=WD,
              num_frames=T, num_inference_steps=3, tile_size=TS, tile_stride=ST, output_type="latents")
    refs = [f.numpy() for f in _frames(2, H, WD, 13)]
    with pytest.raises(ValueError, match="one vace_reference_image"):
        pipe(input_video=video, vace_video=video, vace_reference_image=refs, **kw)
    with pytest.raises(ValueError, match="frames"):
        pipe(input_video=_frames(9, H, WD, 11), **kw)
    with pytest.raises(ValueError, match="frames"):
        pipe(input_video=video[:4], **kw)
    with pytest.raises(ValueError, match="64x96"):
        pipe(input_video=_frames(T, H, WD + 16, 11), **kw)
    with pytest.raises(ValueError, match="not both"):
        pipe(input_video=video, input_latents=x0, **kw)
    with pytest.raises(ValueError, match="input_latents must be"):
        pipe(input_latents=x0[:, :, :1], **kw)
    vae, pipe.vae = pipe.vae, None
    try:
        with pytest.raises(RuntimeError, match="VAE"):
            pipe(input_video=video, **kw)
    finally:
        pipe.vae = vae


def test_graph_replay_on_a_shortened_schedule(tiny):
    cfg, W, Wv, pipe = tiny
    from vstyler import kernels as K
    x0, cp, cn, vc = O.synthetic_inputs(cfg, 5, H, WD)
    noise = O.generate_noise(tuple(x0.shape), 9)
    pipe.scheduler.set_timesteps(3, denoising_strength=0.6, shift=5.0)
    start = K.flow_add_noise(x0.cuda(), noise.cuda(), pipe.scheduler.sigmas[0].item())
    kw = dict(denoising_strength=0.6, num_inference_steps=3)
    eager = pipe.denoise(start, cp.cuda(), cn.cuda(), vc.cuda(), use_graph=False, **kw)
    assert pipe.last_graph is None
    graph = pipe.denoise(start, cp.cuda(), cn.cuda(), vc.cuda(), use_graph=True, **kw)
    assert pipe.last_graph is not None
    assert torch.equal(bits(graph), bits(eager))
    assert not torch.equal(eager, start)


# ------------------------------------------------------------------------------------------ UniPC
def test_unipc_add_noise_then_partial_schedule_bit_exact():
    from vstyler.unipc import FlowUniPCMultistepScheduler
    g = torch.Generator().manual_seed(6)
    x0 = torch.randn(1, 16, 2, 8, 12, generator=g)
    noise = torch.randn(1, 16, 2, 8, 12, generator=g)
    vs = [torch.randn(1, 16, 2, 8, 12, generator=g) for _ in range(3)]
    ref = UniPCOracle(shift=1.0)
    ref.set_timesteps(6, shift=2.0)
    sched = FlowUniPCMultistepScheduler(shift=1.0)
    sched.set_timesteps(6, shift=2.0)
    assert torch.equal(sched.timesteps, ref.timesteps) and len(set(ref.timesteps.tolist())) == 6
    t0 = ref.timesteps[-4]
    sigma = ref.sigmas[(ref.timesteps == t0).nonzero()[0].item()]           # fm_solvers_unipc.py:781-793
    xr = (1 - sigma) * x0 + sigma * noise                                   # :797-799
    xg = sched.add_noise(x0.cuda(), noise.cuda(), torch.IntTensor([t0]))
    assert torch.equal(bits(xg), bits(xr))
    assert sched.step_index is None and sched.last_sample is None and sched.lower_order_nums == 0 \
        and all(m is None for m in sched.model_outputs)
    for v, t in zip(vs, ref.timesteps[-3:]):
        xr = ref.step(v, t, xr)
        xg = sched.step(v.cuda(), t, xg)[0]
        assert torch.equal(bits(xg), bits(xr)), t
    with pytest.raises(ValueError):
        sched.add_noise(x0.cuda().to(BF16), noise.cuda().to(BF16), t0)


UNIPC_KW = dict(vace_scale=0.975, cfg_scale=1.2, sigma_shift=2.0, slg_blocks=(2,))


def _unipc_v2v_chain(W, cfg, noise, x0, cp, cn, vc, n, fwd, back, vace_scale, cfg_scale, sigma_shift, slg_blocks,
                     slg_range=(0.2, 0.7)):
    """text2video.py:347-375 on the oracle's denoise_unipc loop body: add_noise at timesteps[-fwd],
    then timesteps[-back:], a step's SLG fraction being its index in the full schedule."""
    sched = UniPCOracle(shift=1.0)
    sched.set_timesteps(n, shift=sigma_shift)
    sigma = sched.sigmas[(sched.timesteps == sched.timesteps[-fwd]).nonzero()[0].item()]
    x = (1 - sigma) * x0.float() + sigma * noise.float()
    for i in range(n - back, n):
        t = sched.timesteps[i]
        tb = t.reshape(1).to(BF16)
        lat = x.to(BF16)
        vp = O.model_fn(W, cfg, lat, tb, cp, vc, vace_scale)
        skip = tuple(slg_blocks) if slg_range[0] <= i / n <= slg_range[1] else ()
        vn = O.model_fn(W, cfg, lat, tb, cn, vc, vace_scale, skip_blocks=skip)
        v = O.bf(vn.float() + O.bf(cfg_scale * O.bf(vp.float() - vn.float()).float()).float())
        x = sched.step(v.float(), t, x)
    return x.to(BF16)


def _floor_and_ref(fn):
    ref = fn()
    old = O.ACC_DTYPE
    O.ACC_DTYPE = torch.float64
    try:
        ref64 = fn()
    finally:
        O.ACC_DTYPE = old
    return ref, err(ref64, ref)


def test_denoise_unipc_v2v_vs_oracle_chain(tiny):
    cfg, W, Wv, pipe = tiny
    x0, cp, cn, vc = O.synthetic_inputs(cfg, 5, H, WD)
    noise = O.generate_noise(tuple(x0.shape), 9)
    got = pipe.denoise_unipc(noise, cp.cuda(), cn.cuda(), vc.cuda(), num_inference_steps=6, input_latents=x0,
                             forward_step=4, skip_backward_step=3, **UNIPC_KW)
    ref, (fmx, frl) = _floor_and_ref(lambda: _unipc_v2v_chain(W, cfg, noise, x0, cp, cn, vc, 6, 4, 3, **UNIPC_KW))
    mx, rl = err(got, ref)
    print(f"unipc v2v f4 b3 of 6: max-abs {mx:.4g} rel-L2 {rl:.4g} (floor {fmx:.4g} / {frl:.4g})")
    assert rl <= 1.5 * frl + 2e-3 and mx <= 1.5 * fmx + 2e-2
    # forward_step = skip_backward_step = n with sigma_0 < 1 differs from the plain call only by the re-noise
    full = pipe.denoise_unipc(noise, cp.cuda(), cn.cuda(), vc.cuda(), num_inference_steps=6, input_latents=x0,
                              forward_step=6, skip_backward_step=6, **UNIPC_KW)
    assert full.shape == got.shape and not torch.equal(full, got)


def test_denoise_unipc_without_input_latents_unchanged(tiny):
    """The plain sampler still matches oracle.denoise_unipc, with the bound of
    test_unipc_gpu.test_config5_sampler_tiny_vs_oracle."""
    cfg, W, Wv, pipe = tiny
    lat, cp, cn, vc = O.synthetic_inputs(cfg, 5, H, WD)
    got = pipe.denoise_unipc(lat, cp.cuda(), cn.cuda(), vc.cuda(), num_inference_steps=4, **UNIPC_KW)
    ref, (fmx, frl) = _floor_and_ref(lambda: O.denoise_unipc(W, cfg, lat, cp, cn, vc, num_inference_steps=4,
                                                             **UNIPC_KW))
    mx, rl = err(got, ref)
    print(f"unipc plain 4 steps: max-abs {mx:.4g} rel-L2 {rl:.4g} (floor {fmx:.4g} / {frl:.4g})")
    assert rl <= 1.5 * frl + 2e-3 and mx <= 1.5 * fmx + 2e-2
