"""Image-to-video without a GPU: the reference's md5 key-layout table for the image-conditioned DiTs, the
loader's detection, the image embedder's mask / VAE-input layout against a literal restatement of
wan_video_new.py:709-720, and the argument errors of model_fn_wan_video and WanVideoPipeline.__call__."""
import pytest
import torch

import i2v_util as I

BF16 = torch.bfloat16

LAYOUTS = {
    "6bfcfb3b342cb286ce886889d519a77e": dict(dim=5120, in_dim=36, image=True, pos=False, clip=True),
    "6d6ccde6845b95ad9114ab993d917893": dict(dim=1536, in_dim=36, image=True, pos=False, clip=True),
    "3ef3b1f8e1dab83d5b71fd7b617f859f": dict(dim=5120, in_dim=36, image=True, pos=True, clip=True),
    "5b013604280dd715f8457c6ed6d6a626": dict(dim=5120, in_dim=36, image=False, pos=False, clip=False),
    "349723183fc063b2bfc10bb2835cf677": dict(dim=1536, in_dim=48, image=True, pos=False, clip=True),
}
WIDTHS = {5120: dict(ffn_dim=13824, num_heads=40, num_layers=40), 1536: dict(ffn_dim=8960, num_heads=12, num_layers=30)}


@pytest.mark.parametrize("md5", sorted(LAYOUTS))
def test_key_layout_hash(md5):
    """WanModel on the meta device reproduces the reference's hash of sorted 'key:shape' strings, and the
    loader's table carries the reference's flags for it."""
    from vstyler.loader import WAN_COMMON, WAN_I2V_DIT_CONFIGS, hash_state_dict_keys
    from vstyler.models import WanModel
    lay = LAYOUTS[md5]
    cfg = dict(WAN_COMMON, dim=lay["dim"], in_dim=lay["in_dim"], has_image_input=lay["image"],
               has_image_pos_emb=lay["pos"], **WIDTHS[lay["dim"]])
    m = WanModel(device="meta", **cfg)
    assert hash_state_dict_keys(m.state_dict()) == md5
    table = dict(WAN_COMMON, **WAN_I2V_DIT_CONFIGS[md5])
    m2 = WanModel(device="meta", **table)
    assert hash_state_dict_keys(m2.state_dict()) == md5
    assert (m2.in_dim, m2.has_image_input, m2.has_image_pos_emb, m2.require_clip_embedding) == \
        (lay["in_dim"], lay["image"], lay["pos"], lay["clip"])
    assert m2.require_vae_embedding and set(WAN_I2V_DIT_CONFIGS) == set(LAYOUTS)


@pytest.mark.parametrize("image,pos", [(True, False), (True, True), (False, False)])
def test_build_dit_from_shapes(image, pos):
    """A tiny checkpoint outside the hash table: the flags come from its shapes (k_img, emb_pos)."""
    from vstyler.loader import build_dit
    cfg = I.tiny_cfg(num_layers=1, has_image_input=image, has_image_pos_emb=pos)
    W = I.random_weights(cfg)
    dit = build_dit(W, "cpu")
    assert (dit.in_dim, dit.has_image_input, dit.has_image_pos_emb) == (36, image, pos)
    assert hasattr(dit, "img_emb") == image
    sd = dit.state_dict()
    assert set(sd) == set(W)
    for k in W:
        assert torch.equal(sd[k], W[k]), k
    if image:       # k_img | v_img alias one fused buffer after loading
        ca = dit.blocks[0].cross_attn
        assert torch.equal(ca._fw_img, torch.cat([W["blocks.0.cross_attn.k_img.weight"],
                                                  W["blocks.0.cross_attn.v_img.weight"]]))


def test_unsupported_flags_still_raise():
    from vstyler.loader import WAN_COMMON
    from vstyler.models import WanModel
    base = dict(WAN_COMMON, dim=256, ffn_dim=512, num_heads=2, num_layers=1, device="meta")
    for flag in ("has_ref_conv", "add_control_adapter", "seperated_timestep", "fuse_vae_embedding_in_latents"):
        with pytest.raises(NotImplementedError):
            WanModel(**dict(base, **{flag: True}))
    with pytest.raises(ValueError):
        WanModel(**dict(base, in_dim=8))


def test_clip_checkpoint_stays_unrecognised():
    from vstyler.loader import build_dit, build_text_encoder, build_vae
    sd = {"visual.transformer.0.attn.to_qkv.weight": torch.zeros(8, 8), "log_scale": torch.zeros(())}
    assert build_dit(sd, "cpu") is None and build_vae(sd, "cpu") is None and build_text_encoder(sd, "cpu") is None


@pytest.mark.parametrize("num_frames", [5, 9])
@pytest.mark.parametrize("with_end", [False, True])
def test_mask_and_vae_input_layout(num_frames, with_end):
    from vstyler.pipeline import image_mask, image_vae_input
    H, W = 16, 24
    g = torch.Generator().manual_seed(num_frames)
    image = torch.randn((1, 3, H, W), generator=g).to(BF16)
    end = torch.randn((1, 3, H, W), generator=g).to(BF16) if with_end else None
    msk, vin = I.reference_mask_and_vae_input(image, end, num_frames, H, W)
    got_m = image_mask(num_frames, H // 8, W // 8, with_end, dtype=torch.float32)
    assert got_m.shape == (4, (num_frames + 3) // 4, H // 8, W // 8) and got_m.is_contiguous()
    assert torch.equal(got_m, msk)
    # the product's frames are (1, 3, 1, H, W) (preprocess_video of one frame)
    got_v = image_vae_input(image.transpose(0, 1)[None], None if end is None else end.transpose(0, 1)[None],
                            num_frames)
    assert got_v.shape == (1, 3, num_frames, H, W) and got_v.dtype == BF16
    assert torch.equal(got_v[0], vin)
    with pytest.raises(ValueError):
        image_mask(num_frames + 1, 2, 3)


def _tiny(image, in_dim=36):
    cfg = dict(I.tiny_cfg(num_layers=1, has_image_input=image), in_dim=in_dim)
    from vstyler.models import WanModel
    return WanModel(dim=cfg["dim"], in_dim=in_dim, ffn_dim=cfg["ffn_dim"], out_dim=16, text_dim=4096, freq_dim=256,
                    eps=1e-6, patch_size=(1, 2, 2), num_heads=2, num_layers=1, has_image_input=image, device="meta")


def test_model_fn_argument_errors():
    """Raised from the arguments' shapes alone, before any kernel runs."""
    from vstyler import model_fn_wan_video
    lat = torch.zeros(1, 16, 3, 8, 12, dtype=BF16)
    ctx = torch.zeros(1, 64, 4096, dtype=BF16)
    t = torch.tensor([500.0], dtype=BF16)
    clip = torch.zeros(1, 257, 1280, dtype=BF16)
    plain = _tiny(False)
    with pytest.raises(ValueError, match="channels"):          # y channel mismatch
        model_fn_wan_video(plain, latents=lat, timestep=t, context=ctx, y=torch.zeros(1, 16, 3, 8, 12, dtype=BF16))
    with pytest.raises(ValueError, match="y="):                # in_dim > 16 without y
        model_fn_wan_video(plain, latents=lat, timestep=t, context=ctx)
    with pytest.raises(ValueError, match="channels"):          # y on a 16-channel DiT
        model_fn_wan_video(_tiny(False, 16), latents=lat, timestep=t, context=ctx,
                           y=torch.zeros(1, 20, 3, 8, 12, dtype=BF16))
    with pytest.raises(ValueError, match="clip_feature"):      # has_image_input without clip_feature
        model_fn_wan_video(_tiny(True), latents=lat, timestep=t, context=ctx, y=torch.zeros(1, 20, 3, 8, 12, dtype=BF16))
    with pytest.raises(ValueError, match="does not match"):    # y of another size
        model_fn_wan_video(_tiny(True), latents=lat.cpu(), timestep=t, context=ctx, clip_feature=clip,
                           y=torch.zeros(1, 20, 3, 8, 10, dtype=BF16))


def test_pipeline_argument_errors():
    from vstyler import WanVideoPipeline
    img = torch.zeros(64, 96, 3, dtype=torch.uint8)
    emb = torch.zeros(1, 64, 4096, dtype=BF16)
    pipe = WanVideoPipeline(device="cpu")
    pipe.dit = _tiny(False, 16)
    with pytest.raises(ValueError, match="in_dim"):            # input_image on a 16-channel DiT
        pipe(prompt_emb=emb, negative_prompt_emb=emb, input_image=img, height=64, width=96, num_frames=5)
    pipe.dit = _tiny(True)
    with pytest.raises(ValueError, match="clip_feature="):     # a DiT that needs CLIP features, without them
        pipe(prompt_emb=emb, negative_prompt_emb=emb, input_image=img, height=64, width=96, num_frames=5)
    pipe.dit = _tiny(False)
    with pytest.raises(ValueError, match="input_image"):
        pipe(prompt_emb=emb, negative_prompt_emb=emb, end_image=img, height=64, width=96, num_frames=5)
    with pytest.raises(RuntimeError, match="VAE"):             # gets as far as the encode: no VAE loaded
        pipe(prompt_emb=emb, negative_prompt_emb=emb, input_image=img, height=64, width=96, num_frames=5)
    pipe.dit, pipe.dit2 = _tiny(False), _tiny(False, 16)       # both experts take y
    with pytest.raises(ValueError, match="in_dim"):
        pipe(prompt_emb=emb, negative_prompt_emb=emb, input_image=img, height=64, width=96, num_frames=5)
    with pytest.raises(NotImplementedError):
        pipe(prompt_emb=emb, motion_bucket_id=3)
    assert pipe.image_encoder is None
