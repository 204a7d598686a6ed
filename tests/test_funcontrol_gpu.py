"""Wan-Fun control on the GPU: the tiny forward with reference_latents (a has_ref_conv DiT) and with
control_camera_latents_input (a DiT with control_adapter) against tests/funcontrol_util.py within the oracle's
floor, the bit identities (CFG batch == two batch-1 forwards, 4-D == 5-D reference_latents, the plain path
untouched, the adapter twice), the 2-step Euler loops (eager, hipGraph, two experts, sliding window) against
test-side loops, and the pipeline with a tiny VAE against its steps done by hand.

Tiny model of tests/test_i2v_gpu.py: dim 256, 2 heads, 2 layers; latents (1, 16, 3, 8, 12): n = 24 reference
tokens in front of S = 72, 96 rows per sample; images 64x96.  The bound is that file's within_floor."""
import pytest
import torch

import funcontrol_util as FU
import i2v_util as I
from oracle import wan_oracle as O
from oracle import wan_vae_oracle as V
from test_i2v_gpu import bits, within_floor
from vae_util import TINY_VAE

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
H, WD = 64, 96

VARIANTS = {
    "ref48": dict(in_dim=48, has_image_input=True, has_ref_conv=True),            # Fun-Control v1.1
    "ref52": dict(in_dim=52, has_image_input=False, has_ref_conv=True),           # Wan2.2-Fun-A14B-Control
    "cam32": dict(in_dim=32, has_image_input=True, add_control_adapter=True),     # Fun-Control-Camera v1.1
    "cam36": dict(in_dim=36, has_image_input=False, add_control_adapter=True),    # Wan2.2-Fun-A14B-Control-Camera
}


def extra_inputs(seed=17):
    g = torch.Generator("cpu").manual_seed(seed)
    ref = torch.randn((1, 16, 1, 8, 12), generator=g).to(BF16)
    cam = torch.randn((1, 24, 3, H, WD), generator=g).to(BF16)
    return ref, cam


# The floor of within_floor -- the float64 restatement against the float32 one -- is a sample of the bf16
# rounding flips that a change of summation order causes, and it is a small-count sample: the two restatements
# differ by a few fp32 ulp before each rounding, so on a given CPU they may flip no early element at all.  Over
# seeds 5-8 and two timesteps the in_dim 52 model's floor was 0.0019 0.0019 0.0017 0.0015 0.0007 0.0016 0.0012
# and once exactly 0 (rel-L2); for seed 5 one CPU gave 0.0019 and another 0.00015.  A floor without a flip says
# nothing about the flip noise of any other correct summation order (the kernels': 0.002-0.003 on every tiny
# model of this suite), so each variant takes the first weight seed, from 5 up, whose floor is at least
# FLOOR_MIN = 1e-3: two thirds of the median of the eight samples above.  The criterion reads the two
# restatements alone; the bound and the variants are unchanged.
FLOOR_MIN = 1e-3


def conditioned_weights(cfg, forward):
    """(W, ref, ref64) for the first seed in 5..12 whose floor (rel-L2 of ref64 against ref) reaches FLOOR_MIN."""
    from gpu_util import err
    for seed in range(5, 13):
        W = FU.random_weights(cfg, seed=seed)
        ref, ref64 = forward(W), I.with_float64(lambda: forward(W))
        frel = err(ref64, ref)[1]
        print(f"weights seed {seed}: floor rel-L2 {frel:.4g}")
        if frel >= FLOOR_MIN:
            return W, ref, ref64
    raise AssertionError("no seed in 5..12 with a floor of at least FLOOR_MIN")


@pytest.fixture(scope="module")
def models():
    """Per variant: (cfg, W, dit, (lat, y, clip, cp, cn), control kwargs, ref, ref64) -- references once."""
    out = {}
    refl, cam = extra_inputs()
    for name, flags in VARIANTS.items():
        cfg = FU.tiny_cfg(**flags)
        lat, y, clip, cp, cn = I.inputs(cfg)
        if not flags["has_image_input"]:
            clip = None
        ckw = dict(reference_latents=refl) if flags.get("has_ref_conv") else dict(control_camera_latents_input=cam)
        t = torch.tensor([700.0]).to(BF16)

        def run(W):
            return FU.model_fn(W, cfg, lat, t, cp, y, clip, **ckw)
        W, ref, ref64 = conditioned_weights(cfg, run)
        out[name] = (cfg, W, FU.build(cfg, W), (lat, y, clip, cp, cn), ckw, ref, ref64)
    return out


def fwd(dit, lat, ctx, y, clip, t=700.0, **kw):
    from vstyler import model_fn_wan_video
    kw = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    return model_fn_wan_video(dit, latents=lat.cuda(), timestep=torch.tensor([t]).to(BF16).cuda(), context=ctx.cuda(),
                              y=None if y is None else y.cuda(), clip_feature=None if clip is None else clip.cuda(),
                              **kw)


# --------------------------------------------------------------------------------------- single forwards
@pytest.mark.parametrize("variant", ["ref48", "ref52"])
def test_forward_reference_latents(models, variant):
    cfg, W, dit, (lat, y, clip, cp, cn), ckw, ref, ref64 = models[variant]
    got = fwd(dit, lat, cp, y, clip, **ckw).clone()
    assert got.shape == (1, 16, 3, 8, 12)
    within_floor(got, ref, ref64, f"tiny forward, reference_latents [{variant}]")
    r5 = ckw["reference_latents"]
    assert torch.equal(bits(fwd(dit, lat, cp, y, clip, reference_latents=r5[:, :, 0])), bits(got))       # 4-D == 5-D
    # the reference image reaches the output, and a forward without it is another forward
    assert not torch.equal(bits(fwd(dit, lat, cp, y, clip, reference_latents=torch.flip(r5, dims=(4,)))), bits(got))
    assert not torch.equal(bits(fwd(dit, lat, cp, y, clip)), bits(got))


@pytest.mark.parametrize("variant", ["cam32", "cam36"])
def test_forward_camera_control(models, variant):
    cfg, W, dit, (lat, y, clip, cp, cn), ckw, ref, ref64 = models[variant]
    got = fwd(dit, lat, cp, y, clip, **ckw).clone()
    assert got.shape == (1, 16, 3, 8, 12)
    within_floor(got, ref, ref64, f"tiny forward, camera control [{variant}]")
    cam = ckw["control_camera_latents_input"]
    assert not torch.equal(bits(fwd(dit, lat, cp, y, clip, control_camera_latents_input=torch.flip(cam, dims=(2,)))),
                           bits(got))
    assert not torch.equal(bits(fwd(dit, lat, cp, y, clip)), bits(got))


def test_adapter_alone(models):
    """The adapter's output rows (dim 256, T = 3, a 4x6 map) within the floor of its restatement, and twice the
    same bits."""
    cfg, W, dit, _, ckw, _, _ = models["cam32"]
    cam = ckw["control_camera_latents_input"]

    def run():
        return FU.adapter(cam, W).permute(0, 2, 3, 4, 1).reshape(1, 72, cfg["dim"])
    ref, ref64 = run(), I.with_float64(run)
    a = dit.control_adapter(cam.cuda()).clone()
    b = dit.control_adapter(cam.cuda()).clone()
    assert a.shape == (72, cfg["dim"]) and torch.equal(bits(a), bits(b))
    within_floor(a.view(1, 72, -1), ref, ref64, "control adapter alone")


# -------------------------------------------------------------------------------------- bit identities
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_cfg_batch_equals_two_single_forwards(models, variant):
    from vstyler import kernels as K
    from vstyler.options import host_options
    cfg, W, dit, (lat, y, clip, cp, cn), ckw, _, _ = models[variant]
    with K.options(gemm_split=0, attn_split=0, attn_nc=0, attn_impl=8):
        one = torch.cat([fwd(dit, lat, cp, y, clip, **ckw).clone(), fwd(dit, lat, cn, y, clip, **ckw).clone()])
        for prefix in (1, 0):
            with host_options(cfg_prefix=prefix):
                two = fwd(dit, lat, torch.cat([cp, cn]), y, clip, **ckw).clone()
            assert torch.equal(bits(two), bits(one)), prefix
        if "reference_latents" in ckw:         # a reference image per sample: no shared prefix
            r = ckw["reference_latents"]
            r2 = torch.cat([r, torch.flip(r, dims=(3,))])
            per = fwd(dit, lat, torch.cat([cp, cn]), y, clip, reference_latents=r2).clone()
            other = fwd(dit, lat, cn, y, clip, reference_latents=r2[1:]).clone()
            assert torch.equal(bits(per[0:1]), bits(one[0:1])) and torch.equal(bits(per[1:2]), bits(other))


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_without_the_new_inputs_todays_path(models, variant):
    """A has_ref_conv / control_adapter model called without the new inputs == a plain model with the same
    weights, bit for bit, and it never launches a control kernel."""
    from vstyler import kernels as K
    cfg, W, dit, (lat, y, clip, cp, cn), _, _, _ = models[variant]
    plain_cfg = dict(cfg, has_ref_conv=False, add_control_adapter=False)
    plain = FU.build(plain_cfg, {k: v for k, v in W.items() if not k.startswith(("ref_conv", "control_adapter"))})
    want = fwd(plain, lat, torch.cat([cp, cn]), y, clip).clone()
    saved = {n: getattr(K, n) for n in ("ref_rows", "unpatchify_skip", "camera_im2col", "relu")}
    try:
        for n in saved:
            setattr(K, n, lambda *a, **k: (_ for _ in ()).throw(AssertionError("control kernel on the plain path")))
        got = fwd(dit, lat, torch.cat([cp, cn]), y, clip).clone()
    finally:
        for n, f in saved.items():
            setattr(K, n, f)
    assert torch.equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------ Euler loops
def euler_loop(dits, lat, cp, cn, y, clip, ckw, steps=2, boundary=0.875, forward=None):
    """The test-side loop around model_fn_wan_video (tests/test_i2v_gpu.py euler_loop) with the raw control
    inputs handed to every step."""
    from vstyler import kernels as K
    from vstyler import model_fn_wan_video
    from vstyler.flow_match import FlowMatchScheduler
    sch = FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
    sch.set_timesteps(steps, denoising_strength=1.0, shift=5.0)
    x = lat.cuda().to(BF16).contiguous().clone()
    both = torch.cat([cp, cn]).cuda()
    ckw = {k: v.cuda() for k, v in ckw.items()}
    for i, t in enumerate(sch.timesteps):
        dit = dits[1] if len(dits) > 1 and float(t) < boundary * 1000 else dits[0]
        kw = dict(timestep=t.reshape(1).to(BF16).cuda(), context=both, clip_feature=None if clip is None else clip.cuda(),
                  **ckw)
        if forward is None:
            v = model_fn_wan_video(dit, latents=x, y=y.cuda(), **kw)
        else:
            v = forward(dit, x, y.cuda(), kw)
        K.cfg_euler_dev(v[0:1], v[1:2], x, 5.0, torch.tensor([sch.delta(i)], dtype=torch.float32, device="cuda"))
    return x


def oracle_chain(Ws, cfg, lat, cp, cn, y, clip, ckw, steps=2, boundary=875.0):
    sigmas, timesteps = O.set_timesteps(steps, 1.0, 5.0)
    x = lat
    for i, ts in enumerate(timesteps):
        W = Ws[1] if len(Ws) > 1 and float(ts) < boundary else Ws[0]
        t = ts.unsqueeze(0).to(BF16)
        vp = FU.model_fn(W, cfg, x, t, cp, y, clip, **ckw)
        vn = FU.model_fn(W, cfg, x, t, cn, y, clip, **ckw)
        x = O.cfg_euler(vp, vn, x, 5.0, O.euler_delta(sigmas, i))
    return x


@pytest.fixture(scope="module")
def pipe2(models):
    from vstyler import WanVideoPipeline
    cfg, W, dit, inp, ckw, _, _ = models["ref48"]
    W2 = FU.random_weights(cfg, seed=21)
    pipe = WanVideoPipeline(device="cuda")
    pipe.dit = dit
    return pipe, cfg, (W, W2), FU.build(cfg, W2), inp, ckw


def _denoise(pipe, lat, cp, cn, y, clip, ckw, **kw):
    return pipe.denoise(lat, cp.cuda(), cn.cuda(), num_inference_steps=2, y=y, clip_feature=clip, **ckw, **kw)


def test_euler_loop_reference_eager_and_graph(pipe2):
    pipe, cfg, (W, W2), dit2, (lat, y, clip, cp, cn), ckw = pipe2
    want = euler_loop([pipe.dit], lat, cp, cn, y, clip, ckw)
    eager = _denoise(pipe, lat, cp, cn, y, clip, ckw, use_graph=False)
    assert pipe.last_graph is None
    graph = _denoise(pipe, lat, cp, cn, y, clip, ckw, use_graph=True)
    assert pipe.last_graph is not None
    assert torch.equal(bits(eager), bits(want)) and torch.equal(bits(graph), bits(want))

    def chain():
        return oracle_chain([W], cfg, lat, cp, cn, y, clip, ckw)
    within_floor(graph, chain(), I.with_float64(chain), "euler 2 steps, reference_latents")


def test_euler_loop_reference_two_experts(pipe2):
    pipe, cfg, (W, W2), dit2, (lat, y, clip, cp, cn), ckw = pipe2
    pipe.dit2 = dit2
    try:
        want = euler_loop([pipe.dit, dit2], lat, cp, cn, y, clip, ckw)
        eager = _denoise(pipe, lat, cp, cn, y, clip, ckw, use_graph=False)
        graph = _denoise(pipe, lat, cp, cn, y, clip, ckw, use_graph=True)
    finally:
        pipe.dit2 = None
    one = _denoise(pipe, lat, cp, cn, y, clip, ckw, use_graph=False)
    assert torch.equal(bits(eager), bits(want)) and torch.equal(bits(graph), bits(want))
    assert not torch.equal(bits(one), bits(want)), "dit2 (and its ref_conv) was ignored"

    def chain():
        return oracle_chain([W, W2], cfg, lat, cp, cn, y, clip, ckw)
    within_floor(graph, chain(), I.with_float64(chain), "euler 2 steps, reference_latents, two experts")


def test_euler_loop_reference_sliding_window(pipe2):
    """sliding_window_size 2, stride 1 over T = 3 == the test-side tiler (window_util.tile's arithmetic through
    i2v_util.tile_y) whose every window is a forward with the reference rows in front."""
    from vstyler import model_fn_wan_video
    pipe, cfg, (W, W2), dit2, (lat, y, clip, cp, cn), ckw = pipe2

    def tiled(dit, x, yy, kw):
        return I.tile_y(lambda lw, yw: model_fn_wan_video(dit, latents=lw.contiguous(), y=yw.contiguous(), **kw),
                        x, yy, 2, 1)
    want = euler_loop([pipe.dit], lat, cp, cn, y, clip, ckw, forward=tiled)
    kw = dict(sliding_window_size=2, sliding_window_stride=1)
    eager = _denoise(pipe, lat, cp, cn, y, clip, ckw, use_graph=False, **kw)
    graph = _denoise(pipe, lat, cp, cn, y, clip, ckw, use_graph=True, **kw)
    assert torch.equal(bits(eager), bits(want)) and torch.equal(bits(graph), bits(want))
    assert not torch.equal(bits(eager), bits(_denoise(pipe, lat, cp, cn, y, clip, ckw, use_graph=False)))


def test_euler_loop_camera_eager_and_graph(models):
    from vstyler import WanVideoPipeline
    cfg, W, dit, (lat, y, clip, cp, cn), ckw, _, _ = models["cam32"]
    pipe = WanVideoPipeline(device="cuda")
    pipe.dit = dit
    want = euler_loop([dit], lat, cp, cn, y, clip, ckw)
    eager = _denoise(pipe, lat, cp, cn, y, clip, ckw, use_graph=False)
    graph = _denoise(pipe, lat, cp, cn, y, clip, ckw, use_graph=True)
    assert pipe.last_graph is not None
    assert torch.equal(bits(eager), bits(want)) and torch.equal(bits(graph), bits(want))
    with pytest.raises(NotImplementedError, match="sliding"):
        _denoise(pipe, lat, cp, cn, y, clip, ckw, use_graph=False, sliding_window_size=2, sliding_window_stride=1)


# -------------------------------------------------------------------------------------------- Ulysses
def _ulysses_worker(rank, world, port, q):
    try:
        from test_sp import _init
        _init(rank, world, port)
        from sp_util import HostStagedUlysses
        from vstyler import model_fn_wan_video
        cfg = FU.tiny_cfg(**VARIANTS["ref48"])
        dit = FU.build(cfg, FU.random_weights(cfg, seed=5), "cuda:0")
        lat, y, clip, cp, cn = I.inputs(cfg)
        refl, _ = extra_inputs()
        kw = dict(latents=lat.cuda(), timestep=torch.tensor([700.0]).to(BF16).cuda(), context=torch.cat([cp, cn]).cuda(),
                  y=y.cuda(), clip_feature=clip.cuda(), reference_latents=refl.cuda())
        single = model_fn_wan_video(dit, **kw)
        res = {}
        for overlap in (True, False):
            sp = HostStagedUlysses()
            sp.overlap = overlap
            par = model_fn_wan_video(dit, use_unified_sequence_parallel=True, sp_group=sp, **kw)
            torch.cuda.synchronize()
            res[f"overlap{int(overlap)}"] = torch.equal(single.cpu(), par.cpu())
        q.put((rank, res))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))


def test_ulysses_world2_equals_single_gpu_with_reference_rows():
    """96 rows per sample, 48 per rank: the reference rows are ordinary tokens of a grid one frame longer, so
    the world-2 Ulysses forward (tests/sp_util.py's host-staged group, a fresh child process per rank) equals
    the single-GPU forward bit for bit."""
    from test_sp import _spawn
    res = _spawn(_ulysses_worker, 2, timeout=300)
    assert len(res) == 2
    for rank, r in res:
        assert isinstance(r, dict), res
        assert r["overlap1"] is True and r["overlap0"] is True, (rank, r)


# ------------------------------------------------------------------------------------------- pipeline
def _pipe_with_vae(dit):
    from vstyler import WanVideoPipeline, vae
    pipe = WanVideoPipeline(device="cuda")
    pipe.dit = dit
    pipe.vae = vae.WanVideoVAE(z_dim=16, dim=TINY_VAE["dim"], device="cuda").load_state_dict(
        V.random_vae_weights(TINY_VAE, seed=34))
    return pipe


NF, TS, ST = 9, (4, 6), (2, 3)
CALL = dict(height=H, width=WD, num_frames=NF, num_inference_steps=2, seed=3, tile_size=TS, tile_stride=ST)


def test_pipeline_control_video_and_reference_image(models):
    """pipe(control_video=, reference_image=) against its steps done by hand: the two encodes, FunControl's y
    and zero clip_feature (no input_image), then denoise."""
    from vstyler.vae import preprocess_video
    cfg, W, dit, (lat, _, _, cp, cn), _, _, _ = models["ref48"]
    pipe = _pipe_with_vae(dit)
    g = torch.Generator().manual_seed(5)
    video = torch.randint(0, 256, (NF, H, WD, 3), generator=g, dtype=torch.uint8)
    ref_img = torch.randint(0, 256, (H, WD, 3), generator=g, dtype=torch.uint8)
    got = pipe(prompt_emb=cp, negative_prompt_emb=cn, control_video=video, reference_image=ref_img,
               output_type="latents", **CALL)
    control = pipe.vae.encode(preprocess_video(video.cuda()), "cuda", tiled=True, tile_size=TS, tile_stride=ST)
    unit = FU.fun_control(control.cpu(), None, None, cfg["in_dim"], NF, H, WD)
    assert unit["y"].shape == (1, 32, 3, 8, 12) and float(unit["y"][:, 16:].abs().max()) == 0
    assert unit["clip_feature"].shape == (1, 257, 1280) and float(unit["clip_feature"].abs().max()) == 0
    refl = pipe.vae.encode(preprocess_video(ref_img[None].cuda()), "cuda")
    assert refl.shape == (1, 16, 1, 8, 12)
    noise = pipe.generate_noise((1, 16, 3, 8, 12), seed=3)
    want = pipe.denoise(noise, cp.cuda(), cn.cuda(), num_inference_steps=2, y=unit["y"], clip_feature=unit["clip_feature"],
                        reference_latents=refl)
    assert torch.equal(bits(got), bits(want))
    # the precomputed forms give the same call; without the reference image it is another video
    again = pipe(prompt_emb=cp, negative_prompt_emb=cn, control_latents=control, reference_latents=refl,
                 output_type="latents", **CALL)
    assert torch.equal(bits(again), bits(got))
    assert not torch.equal(bits(pipe(prompt_emb=cp, negative_prompt_emb=cn, control_video=video, output_type="latents",
                                     **CALL)), bits(got))


def test_pipeline_camera_control(models):
    """pipe(camera_control_direction="Left", input_image=) on the in_dim 36 model (no CLIP) against its steps by
    hand: the rays through the host path and the kernel, y in the mask + latents form, then denoise; and on the
    in_dim 32 model y is the first frame's latents over zeros."""
    from vstyler.camera import control_camera_latents_input
    from vstyler.vae import preprocess_video
    cfg, W, dit, (lat, _, _, cp, cn), _, _, _ = models["cam36"]
    pipe = _pipe_with_vae(dit)
    g = torch.Generator().manual_seed(7)
    img = torch.randint(0, 256, (H, WD, 3), generator=g, dtype=torch.uint8)
    got = pipe(prompt_emb=cp, negative_prompt_emb=cn, camera_control_direction="Left", input_image=img,
               output_type="latents", **CALL)
    cam = control_camera_latents_input("Left", NF, H, WD, device="cuda")
    assert cam.shape == (1, 24, 3, H, WD)
    y = pipe.encode_input_image(img, None, NF, H, WD, True, TS, ST)
    z = pipe.vae.encode(preprocess_video(img[None].cuda()), "cuda")
    unit_y = FU.camera_y(z.cpu(), lambda: y, cfg["in_dim"], NF, H, WD)                   # in_dim 36: the mask form
    assert unit_y is y and y.shape == (1, 20, 3, 8, 12)
    noise = pipe.generate_noise((1, 16, 3, 8, 12), seed=3)
    want = pipe.denoise(noise, cp.cuda(), cn.cuda(), num_inference_steps=2, y=unit_y, control_camera_latents_input=cam)
    assert torch.equal(bits(got), bits(want))
    other = pipe(prompt_emb=cp, negative_prompt_emb=cn, camera_control_direction="RightDown", input_image=img,
                 output_type="latents", **CALL)
    assert not torch.equal(bits(other), bits(got))
    # in_dim 32: zeros with the untiled encode of the image in latent frame 0 (wan_video_new.py:825-830)
    cfg32, _, dit32, _, _, _, _ = models["cam32"]
    pipe.dit = dit32
    y32 = pipe.encode_camera_y(img, NF, H, WD, True, TS, ST)
    want32 = FU.camera_y(z.cpu(), None, cfg32["in_dim"], NF, H, WD)
    assert torch.equal(bits(y32.cpu()), bits(want32))
