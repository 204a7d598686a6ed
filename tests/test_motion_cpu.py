"""Wan2.2-Animate's motion encoder without a device: the test-side restatement (tests/motion_util.py) against the
reference's recorded outputs (tests/golden/motion_ref.npz, written by tests/golden/make_motion_ref.py from the
reference's Generator(size=64)), the construction of vstyler.motion.MotionEncoder from a key set, and the argument
errors of the adapter, the pipeline and model_fn_wan_video."""
import json
import os

import numpy as np
import pytest
import torch

import motion_util as M

HERE = os.path.dirname(os.path.abspath(__file__))
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(HERE, "golden", "motion_ref.npz"))
    W = M.motion_weights(int(z["size"]), int(z["seed"]))
    for k in z.files:
        if k.startswith("abs_sum."):
            assert W[k[8:]].double().abs().sum().item() == float(z[k]), f"the seeded generator drifted: {k}"
    return {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("abs_sum.")}, W


def test_restatement_float64_equals_the_reference(fixture):
    """Float64 against float64: only the summation order inside the convolutions differs.  Bound: the longest
    dot product has 512 * 16 = 8192 terms and the chain is 4 blocks x 3 convs + stem + 4x4 conv + 5 linears +
    Direction = 20 layers deep, each of which can amplify the error before it by a small factor; 1e5 eps
    (2.2e-11) relative is 8192 x 12 eps with nothing amplified and far below any modelling difference (the
    smallest, a dropped rounding, is ~1e-3)."""
    z, W = fixture
    eps = torch.finfo(torch.float64).eps
    px = M.pure_float64(lambda: M.preprocess(z["frames"]))
    alpha = M.pure_float64(lambda: M.enc_motion(px, W))
    motion = M.pure_float64(lambda: M.get_motion(px, W))
    q = M.pure_float64(lambda: M.direction_q(W[M.PREFIX + "dec.direction.weight"]))
    for name, got, ref in (("enc_motion", alpha, z["enc_motion"]), ("get_motion", motion, z["get_motion"]),
                           ("Q", q, z["Q"])):
        rel, mx = M.err(got, ref)
        print(f"{name}: rel-L2 {rel:.3e} max-abs {mx:.3e}")
        assert got.dtype == torch.float64 and got.shape == ref.shape
        assert rel <= 1e5 * eps, (name, rel)


def test_restatement_bf16_within_the_floor(fixture):
    z, W = fixture
    got = M.get_motion(M.preprocess(z["frames"]), W)
    assert got.dtype == BF16
    M.within_floor(got, z["get_motion"], z["get_motion_bf16"], "bf16 restatement")
    # the constant -1 frame is byte 0, exactly, and frames are independent
    px = M.preprocess(z["frames"])
    assert torch.equal(px[2].float(), torch.full((3, 64, 64), -1.0))
    assert torch.equal(M.get_motion(px[2:3], W).view(torch.int16), got[2:3].view(torch.int16))


def test_restatement_notices_a_dropped_piece(fixture):
    """The floor is not so wide that a wrong encoder passes: without the blur in front of the stride-2 convs, or
    with the bias of FusedLeakyReLU dropped, the bf16 restatement is outside it."""
    z, W = fixture
    px = M.preprocess(z["frames"])
    saved = M.blur

    def no_blur(x, p0, p1, step=1):         # the (H + 1) x (W + 1) input of conv2 by zero padding alone
        return saved(x, p0, p1, step) if (p0, p1) == (1, 1) else torch.nn.functional.pad(x, [1, 0, 1, 0])
    try:
        M.blur = no_blur
        with pytest.raises(AssertionError):
            M.within_floor(M.get_motion(px, W), z["get_motion"], z["get_motion_bf16"], "no blur before conv2")
    finally:
        M.blur = saved
    W0 = {k: (torch.zeros_like(v) if k.endswith("conv1.1.bias") else v) for k, v in W.items()}
    with pytest.raises(AssertionError):
        M.within_floor(M.get_motion(px, W0), z["get_motion"], z["get_motion_bf16"], "conv1 bias dropped")


def _meta_state(shapes):
    return {M.PREFIX + k: torch.empty(s, device="meta") for k, s in shapes.items()}


def test_full_size_key_set_builds_on_meta():
    from vstyler import motion
    keys = json.load(open(os.path.join(HERE, "golden", "animate_keys.json")))
    me = {k: torch.empty(s, device="meta") for k, s in keys.items() if k.startswith(M.PREFIX)}
    assert len(me) == 63
    assert {k[len(M.PREFIX):]: tuple(v.shape) for k, v in me.items()} == M.motion_shapes(512)
    assert motion.size_of(me) == 512
    net = motion.MotionEncoder(me)
    assert net.size == 512 and len(net.blocks) == 7 and net.c0 == 32 and net.motion_dim == 20
    assert [(b["cin"], b["cout"]) for b in net.blocks] == [(32, 64), (64, 128), (128, 256), (256, 512), (512, 512),
                                                           (512, 512), (512, 512)]
    assert tuple(net.stem_w.shape) == (32, 3) and tuple(net.q.shape) == (512, 20) and net.q.dtype == BF16
    assert tuple(net.last.w.shape) == (512, 16 * 512) and net.blocks[0]["conv2"].w.dtype == BF16
    for size in (32, 64):
        assert motion.MotionEncoder(_meta_state(M.motion_shapes(size))).size == size


def test_prepared_weights_are_the_reference_expression():
    """(w.to(bf16) * scale) with that very expression, laid out [cout][ky][kx][cin]; Q = custom_qr on the host."""
    from vstyler import motion
    W = M.motion_weights(32, seed=7)
    net = motion.MotionEncoder(W, device="cpu")
    w = W[M.PREFIX + "enc.net_app.convs.1.conv2.1.weight"]
    want = (w.to(BF16) * (1 / (w.shape[1] * 9) ** 0.5)).permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    assert torch.equal(net.blocks[0]["conv2"].w, want)
    w = W[M.PREFIX + "enc.fc.4.weight"]
    assert torch.equal(net.fc[4][0], w.to(BF16) * (1 / 512 ** 0.5))
    assert torch.equal(net.q, M.direction_q(W[M.PREFIX + "dec.direction.weight"]))
    assert torch.equal(net.blocks[0]["b1"], W[M.PREFIX + "enc.net_app.convs.1.conv1.1.bias"].to(BF16).view(-1))


def test_incomplete_weights_are_not_implemented():
    from vstyler import motion
    from vstyler.models import WanAnimateAdapter
    full = _meta_state(M.motion_shapes(32))
    assert motion.size_of(full) == 32
    for drop in ("enc.fc.3.bias", "enc.net_app.convs.2.skip.1.weight", "dec.direction.weight", "enc.net_app.convs.4.weight"):
        part = {k: v for k, v in full.items() if k != M.PREFIX + drop}
        assert motion.size_of(part) is None, drop
        with pytest.raises(NotImplementedError, match="animate_face_motion="):
            motion.MotionEncoder(part)
    bad = dict(full)
    bad[M.PREFIX + "enc.fc.0.weight"] = torch.empty(512, 256, device="meta")
    assert motion.size_of(bad) is None
    ad = WanAnimateAdapter(dim=256, num_heads=2, num_layers=6, in_dim=512, device="meta")
    assert ad.motion_size() is None
    with pytest.raises(NotImplementedError, match="animate_face_motion="):
        ad.encode_motion(torch.zeros(1, 32, 32, 3, dtype=torch.uint8))
    ad.motion_encoder = full
    assert ad.motion_size() == 32
    assert not any(k.startswith("motion") for k in ad.state_dict())
    assert "motion_net" not in dict(ad.named_modules())
    # another dict drops the encoder built from the previous one; so does load_state_dict
    ad.__dict__["motion_net"] = object()
    ad.motion_encoder = dict(full)
    assert "motion_net" not in ad.__dict__ and ad.motion_size() == 32


def test_argument_errors_of_pipeline_and_model_fn():
    import animate_util as A
    from vstyler.models import WanAnimateAdapter, WanModel
    from vstyler.pipeline import WanVideoPipeline, model_fn_wan_video
    cfg = A.tiny_cfg()
    dit = WanModel(dim=256, in_dim=36, ffn_dim=cfg["ffn_dim"], out_dim=16, text_dim=4096, freq_dim=256, eps=1e-6,
                   patch_size=(1, 2, 2), num_heads=2, num_layers=6, has_image_input=True, device="meta")
    ad = WanAnimateAdapter(dim=cfg["dim"], num_heads=cfg["num_heads"], num_layers=cfg["num_layers"], in_dim=512,
                           device="meta")
    ad.motion_encoder = _meta_state(M.motion_shapes(32))
    pipe = WanVideoPipeline(device="cpu")
    pipe.dit, pipe.animate_adapter = dit, ad
    img = torch.zeros(32, 48, 3, dtype=torch.uint8)
    face = torch.zeros(32, 32, 3, dtype=torch.uint8)
    call = dict(prompt_emb=torch.zeros(1, 8, 4096), negative_prompt_emb=torch.zeros(1, 8, 4096), height=32, width=48,
                num_frames=9, output_type="latents", clip_feature=torch.zeros(1, 257, 1280), input_image=img)
    with pytest.raises(ValueError, match="32 x 32"):
        pipe(animate_face_video=[img] * 5, **call)                              # 32 x 48 frames
    with pytest.raises(ValueError, match="not both"):
        pipe(animate_face_video=[face] * 5, animate_face_motion=torch.zeros(5, 512), **call)
    ad.motion_encoder = {k: v for k, v in ad.motion_encoder.items() if not k.endswith("fc.2.bias")}
    with pytest.raises(NotImplementedError, match="animate_face_motion="):
        pipe(animate_face_video=[face] * 5, **call)
    # model_fn_wan_video follows the same rule
    ad.motion_encoder = _meta_state(M.motion_shapes(32))
    base = dict(latents=torch.zeros(1, 16, 3, 8, 12), timestep=torch.zeros(1), context=torch.zeros(1, 8, 4096))
    with pytest.raises(ValueError, match="32, 32"):
        model_fn_wan_video(dit, animate_adapter=ad, face_pixel_values=torch.zeros(1, 3, 5, 32, 48), **base)
    with pytest.raises(ValueError, match="not both"):
        model_fn_wan_video(dit, animate_adapter=ad, face_pixel_values=torch.zeros(1, 3, 5, 32, 32),
                           animate_face_motion=torch.zeros(1, 5, 512), **base)
    with pytest.raises(NotImplementedError, match="animate_face_motion="):
        model_fn_wan_video(dit, animate_adapter=None, face_pixel_values=torch.zeros(1, 3, 5, 32, 32), **base)
