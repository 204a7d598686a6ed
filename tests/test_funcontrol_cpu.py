"""Wan-Fun control without a GPU: the seven key-layout hashes, the constructor rule, build_dit from shapes,
the argument errors of model_fn_wan_video and the pipeline, the y / clip_feature assembly against the literal
restatement of the three units (tests/funcontrol_util.py), the host camera path against the fixture, the
redirect module -- and the yardstick's own checks: funcontrol_util.model_fn without the new inputs is
i2v_util.model_fn, and a wrong RoPE index for the reference frame is far outside the floor."""
import numpy as np
import pytest
import torch

import funcontrol_util as FU
import i2v_util as I
from gpu_util import err

BF16 = torch.bfloat16

LAYOUTS = {
    "efa44cddf936c70abd0ea28b6cbe946c": dict(dim=5120, in_dim=48, image=True, ref=False, cam=False),
    "70ddad9d3a133785da5ea371aae09504": dict(dim=1536, in_dim=48, image=True, ref=True, cam=False),
    "26bde73488a92e64cc20b0a7485b9e5b": dict(dim=5120, in_dim=48, image=True, ref=True, cam=False),
    "ac6a5aa74f4a0aab6f64eb9a72f19901": dict(dim=1536, in_dim=32, image=True, ref=False, cam=True),
    "b61c605c2adbd23124d152ed28e049ae": dict(dim=5120, in_dim=32, image=True, ref=False, cam=True),
    "2267d489f0ceb9f21836532952852ee5": dict(dim=5120, in_dim=52, image=False, ref=True, cam=False),
    "47dbeab5e560db3180adf51dc0232fb1": dict(dim=5120, in_dim=36, image=False, ref=False, cam=True),
}


@pytest.mark.parametrize("h", sorted(LAYOUTS))
def test_meta_model_reproduces_the_layout_hash(h):
    from vstyler.loader import WAN_COMMON, WAN_FUN_DIT_CONFIGS, build_dit, hash_state_dict_keys
    from vstyler.models import WanModel
    want = LAYOUTS[h]
    cfg = dict(WAN_COMMON, **WAN_FUN_DIT_CONFIGS[h])
    m = WanModel(device="meta", **cfg)
    assert hash_state_dict_keys(m.state_dict()) == h
    assert (m.dim, m.in_dim, m.out_dim, m.has_image_input) == (want["dim"], want["in_dim"], 16, want["image"])
    assert m.has_ref_conv == want["ref"] and (m.control_adapter is not None) == want["cam"]
    assert m.require_clip_embedding == want["image"]
    sd = m.state_dict()
    if want["ref"]:
        assert tuple(sd["ref_conv.weight"].shape) == (m.dim, 16, 2, 2) and tuple(sd["ref_conv.bias"].shape) == (m.dim,)
    if want["cam"]:
        assert tuple(sd["control_adapter.conv.weight"].shape) == (m.dim, 1536, 2, 2)
        for n in ("conv1", "conv2"):
            assert tuple(sd[f"control_adapter.residual_blocks.0.{n}.weight"].shape) == (m.dim, m.dim, 3, 3)
            assert tuple(sd[f"control_adapter.residual_blocks.0.{n}.bias"].shape) == (m.dim,)


def test_tables_stay_apart():
    from vstyler import loader as L
    assert len(L.WAN_FUN_DIT_CONFIGS) == 7 and set(L.WAN_FUN_DIT_CONFIGS) == set(LAYOUTS)
    for t in (L.WAN_DIT_CONFIGS, L.WAN_I2V_DIT_CONFIGS, L.WAN_TI2V_DIT_CONFIGS):
        assert not set(t) & set(L.WAN_FUN_DIT_CONFIGS)


def test_constructor_rule_both_directions():
    from vstyler.loader import WAN_COMMON
    from vstyler.models import SimpleAdapter, WanModel
    base = dict(WAN_COMMON, dim=256, ffn_dim=512, num_heads=2, num_layers=1, device="meta")
    for flag in ("has_ref_conv", "add_control_adapter"):
        for bad in (dict(), dict(in_dim=48, out_dim=48), dict(in_dim=16, out_dim=16), dict(in_dim=32, out_dim=48)):
            with pytest.raises(NotImplementedError, match=flag):
                WanModel(**dict(base, **bad, **{flag: True}))
        m = WanModel(**dict(base, in_dim=32, **{flag: True}))
        assert m.has_ref_conv == (flag == "has_ref_conv")
        assert isinstance(m.control_adapter, SimpleAdapter) == (flag == "add_control_adapter")
    m = WanModel(**dict(base, in_dim=36, add_control_adapter=True, in_dim_control_adapter=6))
    assert tuple(m.control_adapter.conv.weight.shape) == (256, 384, 2, 2)
    plain = WanModel(**dict(base, in_dim=36))
    assert plain.has_ref_conv is False and plain.control_adapter is None and not hasattr(plain, "ref_conv")


@pytest.mark.parametrize("flags", [dict(has_ref_conv=True), dict(add_control_adapter=True),
                                   dict(has_ref_conv=True, add_control_adapter=True)])
def test_build_dit_from_shapes(flags):
    """A tiny checkpoint outside the tables: both key groups are recognised from the shapes, the adapter's input
    channels from conv.weight.shape[1] / 64."""
    from vstyler.loader import build_dit, hash_state_dict_keys, WAN_FUN_DIT_CONFIGS
    cfg = dict(FU.tiny_cfg(in_dim=48, has_image_input=True, num_layers=1, **flags), in_dim_control_adapter=6)
    W = FU.random_weights(cfg, seed=3)
    assert hash_state_dict_keys(W) not in WAN_FUN_DIT_CONFIGS
    dit = build_dit(W, "cpu")
    assert dit is not None and dit.in_dim == 48 and dit.has_image_input
    assert dit.has_ref_conv == bool(flags.get("has_ref_conv"))
    assert (dit.control_adapter is not None) == bool(flags.get("add_control_adapter"))
    if dit.control_adapter is not None:
        assert dit.control_adapter.in_dim == 6
    for k, v in W.items():
        assert torch.equal(dit.state_dict()[k], v), k


def test_fp8_and_lora_leave_the_new_convs_alone():
    from vstyler.lora import hotload_lora
    from vstyler.models import quantize_fp8_
    cfg = FU.tiny_cfg(in_dim=48, has_image_input=False, num_layers=1, has_ref_conv=True, add_control_adapter=True)
    dit = FU.build(cfg, FU.random_weights(cfg, seed=3), "cpu")
    before = {k: v.clone() for k, v in dit.state_dict().items() if k.startswith(("ref_conv", "control_adapter"))}
    assert quantize_fp8_(dit) == 10
    lora = {"ref_conv.lora_A.default.weight": torch.zeros(8, 64, dtype=BF16),
            "ref_conv.lora_B.default.weight": torch.zeros(256, 8, dtype=BF16)}
    assert hotload_lora(dit, lora, fp8_layers="fuse") == 0
    for mod in (dit.ref_conv, dit.control_adapter.conv, dit.control_adapter.residual_blocks[0].conv1):
        assert not hasattr(mod, "weight_fp8") and not hasattr(mod, "lora_A") and mod.weight.dtype == BF16
    for k, v in before.items():
        assert torch.equal(dit.state_dict()[k], v)


def test_redirect_module():
    from diffsynth.models.wan_video_camera_controller import SimpleAdapter
    from vstyler.models import SimpleAdapter as Own
    assert SimpleAdapter is Own
    a = SimpleAdapter(24, 256, device="meta")
    assert sorted(k for k, _ in a.named_parameters()) == sorted(
        ["conv.weight", "conv.bias", "residual_blocks.0.conv1.weight", "residual_blocks.0.conv1.bias",
         "residual_blocks.0.conv2.weight", "residual_blocks.0.conv2.bias"])


# ------------------------------------------------------------------------------------- argument errors
def _meta(in_dim, image=False, **flags):
    cfg = FU.tiny_cfg(in_dim=in_dim, has_image_input=image, num_layers=1, **flags)
    from vstyler.models import WanModel
    return WanModel(dim=cfg["dim"], in_dim=in_dim, ffn_dim=cfg["ffn_dim"], out_dim=16, text_dim=4096, freq_dim=256,
                    eps=1e-6, patch_size=(1, 2, 2), num_heads=2, num_layers=1, has_image_input=image, device="meta",
                    **flags)


def test_model_fn_argument_errors():
    from vstyler import model_fn_wan_video
    from vstyler.models import VaceWanModel
    from vstyler.pipeline import _UNSUPPORTED
    assert "reference_latents" not in _UNSUPPORTED and "control_camera_latents_input" not in _UNSUPPORTED
    assert "motion_bucket_id" in _UNSUPPORTED
    lat = torch.zeros(1, 16, 3, 8, 12, dtype=BF16)
    ctx = torch.zeros(1, 64, 4096, dtype=BF16)
    t = torch.tensor([500.0], dtype=BF16)
    base = dict(latents=lat, timestep=t, context=ctx)
    ref = torch.zeros(1, 16, 1, 8, 12, dtype=BF16)
    cam = torch.zeros(1, 24, 3, 64, 96, dtype=BF16)
    with pytest.raises(ValueError, match="ref_conv"):               # a DiT without ref_conv
        model_fn_wan_video(_meta(48), y=torch.zeros(1, 32, 3, 8, 12, dtype=BF16), reference_latents=ref, **base)
    with pytest.raises(ValueError, match="control_adapter"):        # a DiT without the adapter
        model_fn_wan_video(_meta(32), y=torch.zeros(1, 16, 3, 8, 12, dtype=BF16), control_camera_latents_input=cam,
                           **base)
    refdit = _meta(48, has_ref_conv=True)
    y32 = torch.zeros(1, 32, 3, 8, 12, dtype=BF16)
    for bad in (torch.zeros(1, 16, 2, 8, 12), torch.zeros(1, 16, 8, 10), torch.zeros(1, 8, 8, 12),
                torch.zeros(3, 16, 1, 8, 12), torch.zeros(16, 8, 12)):
        with pytest.raises(ValueError, match="reference_latents"):
            model_fn_wan_video(refdit, y=y32, reference_latents=bad.to(BF16), **base)
    vace = VaceWanModel(vace_layers=(0,), dim=256, num_heads=2, ffn_dim=512, device="meta")
    with pytest.raises(ValueError, match="VACE"):
        model_fn_wan_video(refdit, vace=vace, vace_context=torch.zeros(1, 96, 3, 8, 12, dtype=BF16), y=y32,
                           reference_latents=ref, **base)
    camdit = _meta(32, add_control_adapter=True)
    y16 = torch.zeros(1, 16, 3, 8, 12, dtype=BF16)
    for bad in (torch.zeros(1, 24, 3, 8, 12), torch.zeros(1, 24, 2, 64, 96), torch.zeros(1, 6, 3, 64, 96),
                torch.zeros(2, 24, 3, 64, 96)):
        with pytest.raises(ValueError, match="control_camera_latents_input"):
            model_fn_wan_video(camdit, y=y16, control_camera_latents_input=bad.to(BF16), **base)
    with pytest.raises(NotImplementedError, match="sliding"):      # more than one window
        model_fn_wan_video(camdit, y=y16, control_camera_latents_input=cam, sliding_window_size=2,
                           sliding_window_stride=1, **base)
    with pytest.raises(NotImplementedError, match="motion_bucket_id"):
        model_fn_wan_video(camdit, y=y16, motion_bucket_id=3, **base)


def test_pipeline_argument_errors():
    """Checked before anything is encoded: no VAE is loaded, and none is asked for."""
    from vstyler import WanVideoPipeline
    img = torch.zeros(64, 96, 3, dtype=torch.uint8)
    vid = torch.zeros(5, 64, 96, 3, dtype=torch.uint8)
    emb = torch.zeros(1, 64, 4096, dtype=BF16)
    kw = dict(prompt_emb=emb, negative_prompt_emb=emb, height=64, width=96, num_frames=5)
    pipe = WanVideoPipeline(device="cpu")
    pipe.dit = _meta(32, add_control_adapter=True)
    with pytest.raises(ValueError, match="input_image"):            # camera control without input_image
        pipe(camera_control_direction="Left", **kw)
    pipe.dit = _meta(36)
    with pytest.raises(ValueError, match="control_adapter"):        # camera control on a DiT without the adapter
        pipe(camera_control_direction="Left", input_image=img, **kw)
    with pytest.raises(ValueError, match="ref_conv"):               # reference_image on a DiT without ref_conv
        pipe(reference_image=img, **kw)
    for in_dim in (16, 20):
        pipe.dit = _meta(in_dim)
        with pytest.raises(ValueError, match="control_video"):      # no room for 16 control channels
            pipe(control_video=vid, **kw)
    pipe.dit, pipe.dit2 = _meta(48, has_ref_conv=True), _meta(48)   # both experts need the module
    with pytest.raises(ValueError, match="ref_conv"):
        pipe(reference_image=img, **kw)
    pipe.dit2 = None
    from vstyler.models import WanModel
    pipe.dit = WanModel(dim=256, in_dim=48, ffn_dim=512, out_dim=48, text_dim=4096, freq_dim=256, eps=1e-6,
                        patch_size=(1, 2, 2), num_heads=2, num_layers=1, seperated_timestep=True,
                        require_clip_embedding=False, require_vae_embedding=False, fuse_vae_embedding_in_latents=True,
                        device="meta")
    for arg in (dict(control_video=vid), dict(reference_image=img), dict(camera_control_direction="Left", input_image=img)):
        with pytest.raises(NotImplementedError, match="fuse_vae_embedding_in_latents"):
            pipe(**arg, **dict(kw, output_type="latents"))
    pipe.dit = _meta(48, has_ref_conv=True)
    with pytest.raises(RuntimeError, match="VAE"):                  # gets as far as the encode: no VAE loaded
        pipe(control_video=vid, **kw)
    with pytest.raises(ValueError, match="one of"):
        from vstyler.camera import camera_coordinates
        camera_coordinates("Sideways", 5)


# ------------------------------------------------------------------------------ the y / clip assembly
@pytest.mark.parametrize("in_dim", [48, 52])
@pytest.mark.parametrize("with_image", [False, True])
def test_fun_control_assembly(in_dim, with_image):
    from vstyler.pipeline import fun_control_y
    g = torch.Generator().manual_seed(in_dim)
    nf, Hh, Ww = 9, 64, 96
    control = torch.randn((1, 16, 3, 8, 12), generator=g).to(BF16)
    y = torch.randn((1, 20, 3, 8, 12), generator=g).to(BF16) if with_image else None
    clip = torch.randn((1, 257, 1280), generator=g).to(BF16) if with_image else None
    want = FU.fun_control(control, clip, y, in_dim, nf, Hh, Ww)
    got_y, got_clip = fun_control_y(control, y, clip, in_dim)
    assert got_y.shape == (1, in_dim - 16, 3, 8, 12) and got_y.is_contiguous()
    assert torch.equal(got_y, want["y"]) and torch.equal(got_clip, want["clip_feature"])
    if with_image:          # the last in_dim - 32 channels of the image y: without the mask for 48, all 20 for 52
        assert torch.equal(got_y[:, 16:], y[:, 20 - (in_dim - 32):]) and got_clip is clip
    # y without CLIP features (a DiT without the branch): the reference drops the image y too
    if with_image:
        w2 = FU.fun_control(control, None, y, in_dim, nf, Hh, Ww)
        g2, c2 = fun_control_y(control, y, None, in_dim)
        assert torch.equal(g2, w2["y"]) and torch.equal(c2, w2["clip_feature"]) and float(g2[:, 16:].abs().max()) == 0
    # an explicit clip_feature= is never replaced
    mine = torch.ones((1, 257, 1280), dtype=BF16)
    _, kept = fun_control_y(control, None, mine, in_dim, keep_clip=True)
    assert kept is mine
    with pytest.raises(ValueError, match="control_video"):
        fun_control_y(control, None, None, 24)


@pytest.mark.parametrize("in_dim", [32, 36])
def test_camera_y_assembly(in_dim):
    """encode_camera_y with a stand-in VAE (the encode is a fixed function of the frame's shape) against the
    unit's lines restated; in_dim 36 takes the image embedder's mask + latents y."""
    from vstyler import WanVideoPipeline
    nf, Hh, Ww = 9, 64, 96
    z = torch.arange(16 * 8 * 12, dtype=torch.float32).view(1, 16, 1, 8, 12).to(BF16)

    class FakeVAE:
        z_dim = 16

        def encode(self, videos, device=None, tiled=False, **kw):
            assert tuple(videos.shape) == (1, 3, 1, Hh, Ww) and not tiled
            return z
    pipe = WanVideoPipeline(device="cpu")
    pipe.dit, pipe.vae = _meta(in_dim, add_control_adapter=True), FakeVAE()
    pipe._image_frame = lambda img, name, h, w: torch.zeros(1, 3, 1, h, w, dtype=BF16)
    mask_y = torch.ones(1, 20, 3, 8, 12, dtype=BF16)
    got = pipe.encode_camera_y(object(), nf, Hh, Ww, y=mask_y)
    want = FU.camera_y(z, lambda: mask_y, in_dim, nf, Hh, Ww)
    assert got.shape == (1, in_dim - 16, 3, 8, 12) and torch.equal(got, want)
    if in_dim == 32:
        assert torch.equal(got[:, :, :1], z) and float(got[:, :, 1:].abs().max()) == 0


# -------------------------------------------------------------------------------- the host camera path
def test_host_camera_path_against_the_fixture():
    """camera_matrices (trajectory, intrinsics rescale, relative poses) fed to the float64 restatement, against
    the reference implementation's recorded fp32 output: within the measured fp32 difference (funcontrol_util:
    2.7 * 2^-24; each case's figure is printed), and the default origin's moments are exactly zero."""
    from vstyler.camera import camera_matrices
    for name, (direction, speed, origin, plucker) in FU.fixture().items():
        intr, c2w = camera_matrices(direction, 5, 16, 32, speed, origin)
        assert intr.dtype == np.float32 and intr.shape == (5, 4) and c2w.dtype == np.float32 and c2w.shape == (5, 3, 4)
        assert np.array_equal(c2w[0], np.eye(4, dtype=np.float32)[:3])
        d = np.abs(FU.plucker64(intr, c2w, 16, 32) - plucker.astype(np.float64)).max()
        print(f"{name}: max |float64 restatement - reference fp32| = {d / 2.0 ** -24:.3f} * 2^-24")
        assert d <= FU.MEASURED_FP32_DIFF, name
        if origin is None:
            assert float(np.abs(plucker[..., :3]).max()) == 0.0
        else:
            assert float(np.abs(plucker[..., :3]).max()) > 0.05
    a = camera_matrices("Left", 5, 16, 32)[1]
    b = camera_matrices("Right", 5, 16, 32)[1]
    assert not np.array_equal(a, b) and np.array_equal(a[0], b[0])
    # 480x832: the pose aspect 16:9 is above 832/480, so fx is rescaled; a frame wider than 16:9 rescales fy
    k = camera_matrices("Left", 1, 480, 832)[0][0]
    assert np.isclose(k[0], 480 * (1280 / 720) * 0.532139961) and np.isclose(k[1], 0.946026558 * 480)
    k = camera_matrices("Left", 1, 16, 64)[0][0]
    assert np.isclose(k[0], 0.532139961 * 64) and np.isclose(k[1], 64 / (1280 / 720) * 0.946026558)


def test_grouping_restatement_is_the_stated_rule():
    g = torch.Generator().manual_seed(1)
    p = torch.randn((9, 4, 6, 6), generator=g)
    out = FU.group_in_fours(p, 9)
    assert out.shape == (1, 24, 3, 4, 6)
    for t in range(3):
        for j in range(4):
            for c in range(6):
                assert torch.equal(out[0, c * 4 + j, t], p[max(0, 4 * t + j - 3), ..., c])


# ----------------------------------------------------------------------------- the yardstick's own checks
@pytest.fixture(scope="module")
def ref48():
    cfg = FU.tiny_cfg(in_dim=48, has_image_input=True, has_ref_conv=True)
    W = FU.random_weights(cfg, seed=5)
    return cfg, W, I.inputs(cfg)


def test_restatement_without_the_new_inputs_is_i2v_util(ref48):
    cfg, W, (lat, y, clip, cp, cn) = ref48
    t = torch.tensor([700.0]).to(BF16)
    assert torch.equal(FU.model_fn(W, cfg, lat, t, cp, y, clip), I.model_fn(W, cfg, lat, t, cp, y, clip))


def test_restatement_catches_a_wrong_grid(ref48):
    """The reference frame at RoPE index T instead of 0 (the video frames at 0..T-1): outside within_floor's
    bound (rel <= 1.5 floor_rel + 2e-3, max <= 1.5 floor_max + 2e-2), so the GPU test would catch that grid."""
    cfg, W, (lat, y, clip, cp, cn) = ref48
    t = torch.tensor([700.0]).to(BF16)
    ref_lat = torch.randn((1, 16, 1, 8, 12), generator=torch.Generator().manual_seed(17)).to(BF16)

    def run(**kw):
        return FU.model_fn(W, cfg, lat, t, cp, y, clip, reference_latents=ref_lat, **kw)
    good, good64 = run(), I.with_float64(run)
    wrong = run(ref_rope_index=3)
    fmx, frel = err(good64, good)
    mx, rel = err(wrong, good)
    print(f"wrong grid: max-abs {mx:.4g} rel-L2 {rel:.4g} (floor {fmx:.4g} / {frel:.4g})")
    assert rel > 1.5 * frel + 2e-3 or mx > 1.5 * fmx + 2e-2
    assert torch.equal(run(), good)
    assert torch.equal(FU.model_fn(W, cfg, lat, t, cp, y, clip, reference_latents=ref_lat[:, :, 0]), good)   # 4-D
