"""Wan2.2-Animate's motion encoder on the device (vstyler.motion.MotionEncoder) against the reference's recorded
outputs (tests/golden/motion_ref.npz: Generator(size=64) in float64 and literally in bf16), and the inputs that
reach it: adapter.encode_motion, pipe(animate_face_video=) and model_fn_wan_video(face_pixel_values=) on the tiny
Animate model of tests/test_animate_gpu.py with a size-32 motion encoder."""
import os

import numpy as np
import pytest
import torch

import animate_util as A
import i2v_util as I
import motion_util as M
from oracle import wan_vae_oracle as V
from vae_util import TINY_VAE

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def net64():
    from vstyler.motion import MotionEncoder
    z = np.load(os.path.join(HERE, "golden", "motion_ref.npz"))
    W = M.motion_weights(int(z["size"]), int(z["seed"]))
    return {k: torch.from_numpy(z[k]) for k in z.files}, MotionEncoder(W, device="cuda")


def test_encoder_against_the_reference_fixture(net64):
    """MotionEncoder(size=64) on the fixture's frames within the floor of the reference's own bf16 run; the uint8
    and the planar bf16 input agree to the bit."""
    z, net = net64
    assert net.size == 64 and [(b["cin"], b["cout"]) for b in net.blocks] == [(256, 512)] + [(512, 512)] * 3
    got = net.encode(z["frames"].cuda())
    torch.cuda.synchronize()
    assert got.shape == (3, 512) and got.dtype == BF16
    M.within_floor(got.cpu(), z["get_motion"], z["get_motion_bf16"], "MotionEncoder(64) against the fixture")
    planar = M.preprocess(z["frames"]).permute(1, 0, 2, 3).contiguous()                 # [3, T, S, S]
    assert torch.equal(bits(net.encode(planar.cuda())), bits(got))


def test_chunk_size_and_frame_independence(net64):
    z, net = net64
    frames = torch.cat([z["frames"], M.face_frames(2, 64, seed=47)]).cuda()             # T = 5
    want = bits(net.encode(frames, chunk=5))
    for chunk in (1, 3):
        assert torch.equal(bits(net.encode(frames, chunk=chunk)), want), chunk
    # one working set whatever the chunk sizes were (a ragged last chunk included): six flat trunk buffers, each
    # as large as its level-0 use at the largest chunk, and the tail's seven
    assert len(net.ws.bufs) == 13
    trunk = sum(t.numel() for (name, _, _), t in net.ws.bufs.items() if name.split(".")[1] in ("a", "b", "c1", "bl", "bs", "sk"))
    n, S, c, co = 5, 64, 256, 512
    assert trunk == n * (S * S * c + (S // 2) ** 2 * co + S * S * c + (S + 1) ** 2 * c + (S // 2) ** 2 * c + (S // 2) ** 2 * co)
    # the constant -1 frame alone equals every row of a constant video
    one = net.encode(torch.full((3, 1, 64, 64), -1.0, dtype=BF16, device="cuda"))
    video = net.encode(torch.zeros((4, 64, 64, 3), dtype=torch.uint8, device="cuda"))   # byte 0 is -1
    for t in range(4):
        assert torch.equal(bits(video[t]), bits(one[0])), t
    assert torch.equal(bits(one[0]), want[2])                                           # (the fixture's third frame)
    with pytest.raises(ValueError, match="64 x 64"):
        net.encode(torch.zeros((1, 64, 32, 3), dtype=torch.uint8, device="cuda"))


def test_size_32_loads_and_runs():
    from vstyler.motion import MotionEncoder
    W = M.motion_weights(32, seed=7)
    net = MotionEncoder(W, device="cuda")
    frames = M.face_frames(3, 32, seed=5)
    got = net.encode(frames.cuda()).cpu()
    ref = M.get_motion(M.preprocess(frames), W)
    ref64 = M.pure_float64(lambda: M.get_motion(M.preprocess(frames), W))
    M.within_floor(got, ref64, ref, "MotionEncoder(32) against the restatement")


# ------------------------------------------------------------------------------- the tiny Animate model
H, WD, NF, TS, ST = 32, 48, 9, (4, 6), (2, 3)


@pytest.fixture(scope="module")
def tiny():
    cfg = A.tiny_cfg()
    W = I.random_weights(cfg, seed=5)
    Wa = A.adapter_weights(cfg["dim"], cfg["num_heads"], cfg["num_layers"], in_dim=512)
    dit = I.build(cfg, W)
    ad = A.build_adapter({**Wa, **M.motion_weights(32, seed=7)}, cfg["dim"], cfg["num_heads"], cfg["num_layers"],
                         in_dim=512)
    assert ad.motion_size() == 32 and set(ad.state_dict()) == set(Wa)
    frames = M.face_frames(NF - 4, 32, seed=11)
    other = M.face_frames(NF - 4, 32, seed=12)
    return cfg, dit, ad, frames, other


def test_adapter_encode_motion(tiny):
    _, _, ad, frames, _ = tiny
    got = ad.encode_motion(frames.cuda())
    assert got.shape == (NF - 4, 512) and "motion_net" not in dict(ad.named_modules())
    assert torch.equal(bits(got), bits(ad.motion_net.encode(frames.cuda(), chunk=2)))
    assert not any(k.startswith("motion") for k in ad.state_dict())


def test_model_fn_face_pixel_values(tiny):
    from vstyler import model_fn_wan_video
    cfg, dit, ad, frames, other = tiny
    lat, y, clip, cp, _ = I.inputs(cfg)
    kw = dict(latents=lat.cuda(), timestep=torch.tensor([700.0]).to(BF16).cuda(), context=cp.cuda(), y=y.cuda(),
              clip_feature=clip.cuda(), animate_adapter=ad)

    def planar(f):
        return M.preprocess(f).permute(1, 0, 2, 3).contiguous().cuda()                  # [3, T, 32, 32]
    got = model_fn_wan_video(dit, face_pixel_values=planar(frames)[None], **kw).clone()
    want = model_fn_wan_video(dit, animate_face_motion=ad.encode_motion(planar(frames))[None], **kw).clone()
    assert torch.equal(bits(got), bits(want))
    diff = model_fn_wan_video(dit, face_pixel_values=planar(other)[None], **kw)
    assert not torch.equal(bits(diff), bits(got))
    with pytest.raises(ValueError, match="32, 32"):
        model_fn_wan_video(dit, face_pixel_values=torch.zeros(1, 3, 5, 32, 48, dtype=BF16, device="cuda"), **kw)


def test_pipeline_animate_face_video(tiny):
    """pipe(animate_face_video=frames) with CFG is the animate_face_motion= path on the encoded frames and the
    encoded constant -1 frame, to the bit; other frames give another result."""
    from vstyler import WanVideoPipeline, vae
    cfg, dit, ad, frames, other = tiny
    _, _, clip, cp, cn = I.inputs(cfg)
    pipe = WanVideoPipeline(device="cuda")
    pipe.dit, pipe.animate_adapter = dit, ad
    pipe.vae = vae.WanVideoVAE(z_dim=16, dim=TINY_VAE["dim"], device="cuda").load_state_dict(
        V.random_vae_weights(TINY_VAE, seed=34))
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (H, WD, 3), generator=g, dtype=torch.uint8)
    pose = torch.randn((1, 16, 2, 4, 6), generator=g).to(BF16)
    call = dict(prompt_emb=cp, negative_prompt_emb=cn, input_image=img, pose_latents=pose, clip_feature=clip,
                output_type="latents", height=H, width=WD, num_frames=NF, num_inference_steps=2, seed=3, tile_size=TS,
                tile_stride=ST)
    got = pipe(animate_face_video=[f for f in frames], **call)
    assert got.shape == (1, 16, 2, 4, 6)
    motion = ad.encode_motion(frames.cuda())
    uncond = ad.encode_motion(torch.full((3, 1, 32, 32), -1.0, dtype=BF16, device="cuda"))[0]
    want = pipe(animate_face_motion=motion, animate_face_motion_uncond=uncond, **call)
    assert torch.equal(bits(got), bits(want))
    assert not torch.equal(bits(pipe(animate_face_video=other, **call)), bits(got))
    # frames that are not size x size
    with pytest.raises(ValueError):
        pipe(animate_face_video=frames[:, :, :16], **call)
