"""Wan2.2-Animate on the GPU: the face encoder and one FaceBlock against the reference's own float64 output
(tests/golden/animate_ref.npz), the tiny forward with pose latents and face motion against
tests/animate_util.py within the oracle's floor, the bit identities (CFG batch == two batch-1 forwards with
their own K / V, the plain path untouched), the 2-step Euler loop (eager == hipGraph, a second call with
another motion and pose), the world-2 Ulysses forward, and the pipeline with a tiny VAE and CLIP against its
steps done by hand.

Tiny model: tests/test_i2v_gpu.py's (dim 256, 2 heads, in_dim 36, image input) with 6 layers -- fuser blocks
after blocks 0 and 5; latents (1, 16, 3, 8, 12): 3 frames of 4 x 6 tokens; T_face = 5 (-> 2 + 1 frames of 5
motion tokens).  The bound is test_i2v_gpu.py's within_floor."""
import os

import numpy as np
import pytest
import torch

import animate_util as A
import i2v_util as I
from oracle import wan_oracle as O
from oracle import wan_vae_oracle as V
from test_i2v_gpu import bits, within_floor
from vae_util import TINY_VAE

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
IN_DIM = 32                 # the tiny face encoder's motion width


@pytest.fixture(scope="module")
def model():
    """(cfg, W, Wa, dit, adapter, inputs, (pose, motion, uncond), ref, ref64): the references computed once."""
    cfg = A.tiny_cfg()
    W = I.random_weights(cfg, seed=5)
    Wa = A.adapter_weights(cfg["dim"], cfg["num_heads"], cfg["num_layers"], in_dim=IN_DIM)
    lat, y, clip, cp, cn = I.inputs(cfg)
    pose, motion = A.animate_inputs(in_dim=IN_DIM)
    uncond = A.animate_inputs(in_dim=IN_DIM, seed=77)[1][:, 0]              # one vector [1, C]
    t = torch.tensor([700.0]).to(BF16)

    def run():
        return A.model_fn(W, Wa, cfg, lat, t, cp, y, clip, pose_latents=pose, motion=motion)
    ref, ref64 = run(), I.with_float64(run)
    dit = I.build(cfg, W)
    ad = A.build_adapter(Wa, cfg["dim"], cfg["num_heads"], cfg["num_layers"], in_dim=IN_DIM)
    return cfg, W, Wa, dit, ad, (lat, y, clip, cp, cn), (pose, motion, uncond), ref, ref64


def fwd(dit, lat, ctx, y, clip, t=700.0, **kw):
    from vstyler import model_fn_wan_video
    kw = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    return model_fn_wan_video(dit, latents=lat.cuda(), timestep=torch.tensor([t]).to(BF16).cuda(), context=ctx.cuda(),
                              y=y.cuda(), clip_feature=clip.cuda(), **kw)


# ------------------------------------------------------------------------------------------ the fixture
def test_face_encoder_and_face_block_against_the_reference_fixture():
    from vstyler.models import RunCtx, Workspace
    fx = np.load(os.path.join(HERE, "golden", "animate_ref.npz"))
    W = A.adapter_weights(256, 2, 6, in_dim=32, seed=int(fx["seed"]))
    ad = A.build_adapter(W, 256, 2, 6, in_dim=32)
    g = torch.Generator().manual_seed(31)
    motion = torch.randn((1, 9, 32), generator=g).to(BF16)
    x = torch.randn((1, 24, 256), generator=g).to(BF16)
    ws = Workspace("cuda")
    tok = ad.face_encoder(motion.cuda(), ws)
    assert tok.shape == (1, 3, 5, 256)
    want = torch.from_numpy(fx["face_encoder"])
    within_floor(tok, A.face_encoder(motion, W), want, "face encoder against the fixture")
    assert torch.equal(bits(tok[:, :, 4]), bits(W["face_encoder.padding_tokens"].view(1, 1, 256).expand(1, 3, 256)))
    # one FaceBlock on the fixture's own motion tensor (rounded to bf16) behind a zero frame
    mv = torch.cat([torch.zeros_like(want[:, :1]), want], dim=1).to(BF16)
    kv = ad.face_kv(mv.cuda(), ws)
    assert len(kv) == 2 and kv[0].shape == (1, 4 * 5, 512)
    rc = RunCtx(1, 24, (4, 2, 3), None, None, 0, ws)
    out = ad.after_block(0, x.cuda().view(24, 256).clone(), kv, rc).view(1, 24, 256)
    ref = O.add(A.face_block(x, mv, W, "face_adapter.fuser_blocks.0.", 2), x)
    ref64 = x.double() + torch.from_numpy(fx["face_block"])
    within_floor(out, ref, ref64, "x + FaceBlock(x) against the fixture")
    assert not torch.equal(bits(out), bits(x))
    # a block index that is no multiple of 5 leaves x alone
    same = ad.after_block(3, x.cuda().view(24, 256).clone(), kv, rc)
    assert torch.equal(bits(same.view(1, 24, 256)), bits(x))


def test_motion_tokens_zero_frame_and_kv_of_it(model):
    """The zero frame in front stays zero through pre_norm_motion, so its keys and values are linear1_kv's bias
    (K through k_norm): the same rows for every motion."""
    from vstyler.models import Workspace
    cfg, W, Wa, dit, ad, _, (pose, motion, uncond), _, _ = model
    ws = Workspace("cuda")
    mv = ad.motion_tokens(motion.cuda(), ws)
    assert mv.shape == (1, 3, 5, 256) and float(mv[:, 0].abs().max()) == 0
    within_floor(mv, A.motion_tokens(motion, Wa), I.with_float64(lambda: A.motion_tokens(motion, Wa)), "motion tokens")
    a = [k.clone() for k in ad.face_kv(mv, ws)]
    b = [k.clone() for k in ad.face_kv(ad.motion_tokens(torch.flip(motion, dims=(1,)).cuda(), ws), ws)]
    for ka, kb in zip(a, b):
        assert torch.equal(bits(ka[:, :5]), bits(kb[:, :5])) and not torch.equal(bits(ka[:, 5:]), bits(kb[:, 5:]))


# ------------------------------------------------------------------------------------- single forwards
def test_forward_with_pose_and_motion(model):
    from gpu_util import err
    cfg, W, Wa, dit, ad, (lat, y, clip, cp, cn), (pose, motion, uncond), ref, ref64 = model
    got = fwd(dit, lat, cp, y, clip, animate_adapter=ad, pose_latents=pose, animate_face_motion=motion).clone()
    assert got.shape == (1, 16, 3, 8, 12)
    within_floor(got, ref, ref64, "tiny forward, pose + face motion")
    # far more than the floor away from the forward without them, and each input reaches the output
    plain = fwd(dit, lat, cp, y, clip).clone()
    floor = err(ref64, ref)[1]
    away = err(plain, ref)[1]
    print(f"without the adapter: rel-L2 {away:.4g} from the reference (floor {floor:.4g})")
    assert away > 10 * (1.5 * floor + 2e-3)
    only_pose = fwd(dit, lat, cp, y, clip, animate_adapter=ad, pose_latents=pose).clone()
    only_face = fwd(dit, lat, cp, y, clip, animate_adapter=ad, animate_face_motion=motion).clone()
    for other in (only_pose, only_face, plain):
        assert not torch.equal(bits(other), bits(got))
    assert not torch.equal(bits(only_pose), bits(plain)) and not torch.equal(bits(only_face), bits(plain))
    ref_pose = A.model_fn(W, Wa, cfg, lat, torch.tensor([700.0]).to(BF16), cp, y, clip, pose_latents=pose)
    ref_face = A.model_fn(W, Wa, cfg, lat, torch.tensor([700.0]).to(BF16), cp, y, clip, motion=motion)
    assert err(only_pose, ref_pose)[1] <= 1.5 * floor + 2e-3 and err(only_face, ref_face)[1] <= 1.5 * floor + 2e-3
    with pytest.raises(ValueError, match="latent frames"):
        fwd(dit, lat, cp, y, clip, animate_adapter=ad, animate_face_motion=torch.cat([motion, motion], dim=1))
    with pytest.raises(ValueError, match="pose_latents"):
        fwd(dit, lat, cp, y, clip, animate_adapter=ad, pose_latents=torch.cat([pose, pose], dim=2))


def test_cfg_batch_equals_two_single_forwards_with_their_own_kv(model):
    from vstyler import kernels as K
    from vstyler.options import host_options
    cfg, W, Wa, dit, ad, (lat, y, clip, cp, cn), (pose, motion, uncond), _, _ = model
    mu = uncond.view(1, 1, IN_DIM).expand(1, motion.shape[1], IN_DIM).contiguous()
    kw = dict(animate_adapter=ad, pose_latents=pose)
    with K.options(gemm_split=0, attn_split=0, attn_nc=0, attn_impl=8):
        one = torch.cat([fwd(dit, lat, cp, y, clip, animate_face_motion=motion, **kw).clone(),
                         fwd(dit, lat, cn, y, clip, animate_face_motion=mu, **kw).clone()])
        for prefix in (1, 0):
            with host_options(cfg_prefix=prefix):
                two = fwd(dit, lat, torch.cat([cp, cn]), y, clip, animate_face_motion=torch.cat([motion, mu]), **kw).clone()
            assert torch.equal(bits(two), bits(one)), prefix
        swapped = fwd(dit, lat, torch.cat([cp, cn]), y, clip, animate_face_motion=torch.cat([mu, motion]), **kw).clone()
        assert not torch.equal(bits(swapped[0:1]), bits(one[0:1])) and not torch.equal(bits(swapped[1:2]), bits(one[1:2]))


def test_without_the_new_inputs_todays_path(model):
    """With the adapter handed over but neither input, the forward is today's, bit for bit, and no animate
    kernel is launched."""
    from vstyler import kernels as K
    cfg, W, Wa, dit, ad, (lat, y, clip, cp, cn), _, _, _ = model
    want = fwd(dit, lat, torch.cat([cp, cn]), y, clip).clone()
    saved = {n: getattr(K, n) for n in ("face_attn", "head_rmsnorm", "ln_silu")}
    try:
        for n in saved:
            setattr(K, n, lambda *a, **k: (_ for _ in ()).throw(AssertionError("animate kernel on the plain path")))
        got = fwd(dit, lat, torch.cat([cp, cn]), y, clip, animate_adapter=ad).clone()
    finally:
        for n, f in saved.items():
            setattr(K, n, f)
    assert torch.equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------ Euler loop
def euler_loop(dit, ad, lat, cp, cn, y, clip, pose, motion, uncond, steps=2):
    """The test-side loop around model_fn_wan_video with the raw animate inputs handed to every step."""
    from vstyler import kernels as K
    from vstyler import model_fn_wan_video
    from vstyler.flow_match import FlowMatchScheduler
    sch = FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
    sch.set_timesteps(steps, denoising_strength=1.0, shift=5.0)
    x = lat.cuda().to(BF16).contiguous().clone()
    both = torch.cat([cp, cn]).cuda()
    m2 = torch.cat([motion, uncond.view(1, 1, -1).expand(1, motion.shape[1], motion.shape[2])]).cuda()
    for i, t in enumerate(sch.timesteps):
        v = model_fn_wan_video(dit, animate_adapter=ad, latents=x, y=y.cuda(), timestep=t.reshape(1).to(BF16).cuda(),
                               context=both, clip_feature=clip.cuda(), pose_latents=pose.cuda(), animate_face_motion=m2)
        K.cfg_euler_dev(v[0:1], v[1:2], x, 5.0, torch.tensor([sch.delta(i)], dtype=torch.float32, device="cuda"))
    return x


def test_euler_loop_eager_graph_and_a_second_call(model):
    from vstyler import WanVideoPipeline
    cfg, W, Wa, dit, ad, (lat, y, clip, cp, cn), (pose, motion, uncond), _, _ = model
    pipe = WanVideoPipeline(device="cuda")
    pipe.dit, pipe.animate_adapter = dit, ad

    def denoise(pose, motion, **kw):
        return pipe.denoise(lat, cp.cuda(), cn.cuda(), num_inference_steps=2, y=y, clip_feature=clip, pose_latents=pose,
                            animate_face_motion=motion, animate_face_motion_uncond=uncond, **kw).clone()
    want = euler_loop(dit, ad, lat, cp, cn, y, clip, pose, motion, uncond)
    eager = denoise(pose, motion, use_graph=False)
    assert pipe.last_graph is None
    graph = denoise(pose, motion, use_graph=True)
    assert pipe.last_graph is not None
    assert torch.equal(bits(eager), bits(want)) and torch.equal(bits(graph), bits(want))
    # a second call on the same pipe with another motion and pose: that call's result, not stale K / V or rows
    pose2, motion2 = A.animate_inputs(in_dim=IN_DIM, seed=99)
    want2 = euler_loop(dit, ad, lat, cp, cn, y, clip, pose2, motion2, uncond)
    assert not torch.equal(bits(want2), bits(want))
    assert torch.equal(bits(denoise(pose2, motion2, use_graph=True)), bits(want2))
    assert torch.equal(bits(denoise(pose2, motion2, use_graph=False)), bits(want2))
    assert torch.equal(bits(denoise(pose, motion, use_graph=True)), bits(want))
    with pytest.raises(ValueError, match="animate_face_motion_uncond"):
        pipe.denoise(lat, cp.cuda(), cn.cuda(), num_inference_steps=2, y=y, clip_feature=clip, animate_face_motion=motion)
    # cfg_scale 1: a batch-1 loop, no unconditioned motion needed
    one = pipe.denoise(lat, cp.cuda(), None, num_inference_steps=2, y=y, clip_feature=clip, cfg_scale=1.0,
                       pose_latents=pose, animate_face_motion=motion)
    assert one.shape == lat.shape and not torch.equal(bits(one), bits(want))


def test_fp8_dit_layers_leave_the_adapter_bf16(model):
    """quantize_fp8_ converts the DiT's block Linears only: the adapter keeps its bf16 weights, its once-per-call
    tensors are the bf16 DiT's to the bit, and the fp8 forward with the adapter runs (CFG batch == two batch-1
    forwards there too)."""
    from vstyler import kernels as K
    from vstyler.models import Workspace, quantize_fp8_
    cfg, W, Wa, _, ad, (lat, y, clip, cp, cn), (pose, motion, uncond), _, _ = model
    ws = Workspace("cuda")
    before = [k.clone() for k in ad.face_kv(ad.motion_tokens(motion.cuda(), ws), ws)]
    dit8 = I.build(cfg, W)
    assert quantize_fp8_(dit8) == 10 * cfg["num_layers"]
    assert all(getattr(m, "weight_fp8", None) is None for m in ad.modules())
    after = ad.face_kv(ad.motion_tokens(motion.cuda(), ws), ws)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(before, after))
    kw = dict(animate_adapter=ad, pose_latents=pose, animate_face_motion=motion)
    with K.options(gemm_split=0, attn_split=0, attn_nc=0, attn_impl=8):
        one = torch.cat([fwd(dit8, lat, cp, y, clip, **kw).clone(), fwd(dit8, lat, cn, y, clip, **kw).clone()])
        two = fwd(dit8, lat, torch.cat([cp, cn]), y, clip, **kw).clone()
    assert torch.isfinite(two.float()).all() and torch.equal(bits(two), bits(one))
    assert not torch.equal(bits(two), bits(fwd(dit8, lat, torch.cat([cp, cn]), y, clip)))


# -------------------------------------------------------------------------------------------- Ulysses
def _ulysses_worker(rank, world, port, q):
    try:
        from test_sp import _init
        _init(rank, world, port)
        from sp_util import HostStagedUlysses
        from vstyler import model_fn_wan_video
        cfg = A.tiny_cfg()
        dit = I.build(cfg, I.random_weights(cfg, seed=5), "cuda:0")
        Wa = A.adapter_weights(cfg["dim"], cfg["num_heads"], cfg["num_layers"], in_dim=IN_DIM)
        ad = A.build_adapter(Wa, cfg["dim"], cfg["num_heads"], cfg["num_layers"], in_dim=IN_DIM, device="cuda:0")
        lat, y, clip, cp, cn = I.inputs(cfg)
        pose, motion = A.animate_inputs(in_dim=IN_DIM)
        m2 = torch.cat([motion, torch.flip(motion, dims=(1,))])
        kw = dict(latents=lat.cuda(), timestep=torch.tensor([700.0]).to(BF16).cuda(), context=torch.cat([cp, cn]).cuda(),
                  y=y.cuda(), clip_feature=clip.cuda(), animate_adapter=ad, pose_latents=pose.cuda(),
                  animate_face_motion=m2.cuda())
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


def test_ulysses_world2_equals_single_gpu():
    """72 rows per sample, 36 per rank: rank 1 starts inside latent frame 1 (token_offset 36, 24 tokens per
    frame), so the face attention's frame index crosses a frame inside its rows.  The operator is row-local:
    the world-2 forward (tests/sp_util.py's host-staged group, a fresh child process per rank) equals the
    single-GPU forward bit for bit, under test_funcontrol_gpu.py's rule."""
    from test_sp import _spawn
    res = _spawn(_ulysses_worker, 2, timeout=300)
    assert len(res) == 2
    for rank, r in res:
        assert isinstance(r, dict), res
        assert r["overlap1"] is True and r["overlap0"] is True, (rank, r)


# ------------------------------------------------------------------------------------------- pipeline
H, WD, NF, TS, ST = 32, 48, 9, (4, 6), (2, 3)
CALL = dict(height=H, width=WD, num_frames=NF, num_inference_steps=2, seed=3, tile_size=TS, tile_stride=ST)


def test_pipeline_end_to_end(model):
    """pipe(animate_pose_video=, animate_face_motion=, input_image=) at 32x48x9 with a tiny VAE and CLIP against
    its steps done by hand; the inpaint / mask form of y; the output's frame count (frame 0 dropped)."""
    import clip_util as C
    from vstyler import WanVideoPipeline, vae
    from vstyler.vae import preprocess_video
    cfg, W, Wa, dit, ad, (_, _, _, cp, cn), (_, motion, uncond), _, _ = model
    pipe = WanVideoPipeline(device="cuda")
    pipe.dit, pipe.animate_adapter = dit, ad
    pipe.vae = vae.WanVideoVAE(z_dim=16, dim=TINY_VAE["dim"], device="cuda").load_state_dict(
        V.random_vae_weights(TINY_VAE, seed=34))
    pipe.image_encoder = C.build(C.WIDE1, C.random_weights(C.WIDE1, seed=23, extras=False))
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (H, WD, 3), generator=g, dtype=torch.uint8)
    pose_video = torch.randint(0, 256, (NF - 4, H, WD, 3), generator=g, dtype=torch.uint8)
    bg_video = torch.randint(0, 256, (NF - 4, H, WD, 3), generator=g, dtype=torch.uint8)
    mask_video = (torch.rand((NF - 4, H // 8, WD // 8, 1), generator=g) < 0.5).to(torch.uint8) * 255
    mask_video = mask_video.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2).expand(NF - 4, H, WD, 3).contiguous()
    akw = dict(animate_face_motion=motion[0], animate_face_motion_uncond=uncond[0])
    got = pipe(prompt_emb=cp, negative_prompt_emb=cn, input_image=img, animate_pose_video=pose_video,
               output_type="latents", **akw, **CALL)
    assert got.shape == (1, 16, 2, 4, 6)                                    # T = 3 latent frames, frame 0 dropped
    # by hand: the pose encode, y and the CLIP feature of input_image as today, noise of T = 3 frames, denoise
    pose = pipe.vae.encode(preprocess_video(pose_video.cuda()), "cuda", tiled=True, tile_size=TS, tile_stride=ST)
    assert pose.shape == (1, 16, 2, 4, 6)
    y = pipe.encode_input_image(img, None, NF, H, WD, True, TS, ST)
    clip = pipe.encode_clip_image(img, None, H, WD)
    noise = pipe.generate_noise((1, 16, 3, 4, 6), seed=3)
    want = pipe.denoise(noise, cp.cuda(), cn.cuda(), num_inference_steps=2, y=y, clip_feature=clip, pose_latents=pose,
                        animate_face_motion=motion, animate_face_motion_uncond=uncond)
    assert torch.equal(bits(got), bits(want[:, :, 1:]))
    again = pipe(prompt_emb=cp, negative_prompt_emb=cn, input_image=img, pose_latents=pose, output_type="latents",
                 **akw, **CALL)
    assert torch.equal(bits(again), bits(got))
    # the inpaint / mask form of y
    inp = pipe(prompt_emb=cp, negative_prompt_emb=cn, input_image=img, animate_pose_video=pose_video,
               animate_inpaint_video=bg_video, animate_mask_video=mask_video, output_type="latents", **akw, **CALL)
    y2 = pipe.encode_animate_inpaint(img, bg_video, mask_video, H, WD, NF, True, TS, ST)
    bgl = pipe.vae.encode(preprocess_video(bg_video.cuda()), "cuda", tiled=True, tile_size=TS, tile_stride=ST)
    refl = pipe.vae.encode(preprocess_video(img[None].cuda()), "cuda", tiled=True, tile_size=TS, tile_stride=ST)
    pre = (mask_video[..., 0].to(BF16) * (1.0 / 255))[None, None]
    assert torch.equal(bits(y2), bits(A.inpaint_y(refl[0].cpu(), bgl[0].cpu(), pre)))
    assert y2.shape == (1, 20, 3, 4, 6) and not torch.equal(bits(y2), bits(y))
    want2 = pipe.denoise(noise, cp.cuda(), cn.cuda(), num_inference_steps=2, y=y2, clip_feature=clip, pose_latents=pose,
                         animate_face_motion=motion, animate_face_motion_uncond=uncond)
    assert torch.equal(bits(inp), bits(want2[:, :, 1:])) and not torch.equal(bits(inp), bits(got))
    # decoded: num_frames - 4 frames
    video = pipe(prompt_emb=cp, negative_prompt_emb=cn, input_image=img, pose_latents=pose, **akw, **CALL)
    assert len(video) == NF - 4
    with pytest.raises(ValueError, match="num_frames - 4"):
        pipe(prompt_emb=cp, negative_prompt_emb=cn, input_image=img, animate_pose_video=pose_video[:4],
             output_type="latents", **akw, **CALL)
