"""Wan2.2-TI2V-5B without a GPU: the checkpoint's key hash and config, the key layout of the product
model, the yardstick (tests/ti2v_util.py) against the oracle, the latent geometry, and every argument the
first-frame path refuses."""
import pytest
import torch

import ti2v_util as T
from oracle import wan_oracle as O

BF16 = torch.bfloat16


def test_5b_layout_hash_and_loader_config():
    from vstyler import loader
    assert O.hash_state_dict_keys(O.dit_param_shapes(T.TI2V_5B)) == T.TI2V_5B_HASH
    cfg = dict(loader.WAN_COMMON, **loader.WAN_TI2V_DIT_CONFIGS[T.TI2V_5B_HASH])
    want = dict(has_image_input=False, patch_size=(1, 2, 2), in_dim=48, dim=3072, ffn_dim=14336, freq_dim=256,
                text_dim=4096, out_dim=48, num_heads=24, num_layers=30, eps=1e-6, seperated_timestep=True,
                require_clip_embedding=False, require_vae_embedding=False, fuse_vae_embedding_in_latents=True)
    assert cfg == want      # wan_video_dit.py:678-696
    for table in (loader.WAN_DIT_CONFIGS, loader.WAN_I2V_DIT_CONFIGS):
        assert T.TI2V_5B_HASH not in table


def test_meta_model_has_the_5b_key_layout():
    from vstyler import loader
    from vstyler.models import WanModel
    cfg = dict(loader.WAN_COMMON, **loader.WAN_TI2V_DIT_CONFIGS[T.TI2V_5B_HASH])
    dit = WanModel(device="meta", **cfg)
    assert dit.seperated_timestep and dit.fuse_vae_embedding_in_latents
    assert not dit.require_vae_embedding and not dit.require_clip_embedding
    shapes = {k: tuple(v.shape) for k, v in dit.state_dict().items()}
    assert shapes == {k: tuple(v) for k, v in O.dit_param_shapes(T.TI2V_5B).items()}
    assert O.hash_state_dict_keys(shapes) == T.TI2V_5B_HASH


def test_model_still_refuses_the_other_layouts():
    from vstyler.models import WanModel
    kw = dict(dim=256, in_dim=48, ffn_dim=512, out_dim=48, text_dim=4096, freq_dim=256, eps=1e-6, patch_size=(1, 2, 2),
              num_heads=2, num_layers=1, device="meta")
    for flag in ("has_ref_conv", "add_control_adapter"):
        with pytest.raises(NotImplementedError, match=flag):
            WanModel(**kw, **{flag: True})


def test_restatement_with_one_timestep_equals_the_oracle():
    """The yardstick's own check: with frame 0's tokens forced to the step's timestep the per-token path
    is the oracle's forward, bit for bit."""
    cfg = T.TINY_TI2V
    W = T.random_weights(cfg)
    lat, _, cp, cn = T.inputs(cfg, T=2, h=4, w=4)
    t = torch.tensor([637.0]).to(BF16)
    ctx = torch.cat([cp, cn])
    got = T.model_fn(W, cfg, lat, t, ctx, first=float(t))
    ref = O.model_fn(W, cfg, lat.expand(2, *lat.shape[1:]), t.expand(2), ctx)
    assert got.shape == ref.shape == (2, 48, 2, 4, 4)
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    seg = T.model_fn(W, cfg, lat, t, ctx)
    assert not torch.equal(seg[:, :, 1:], ref[:, :, 1:])      # the segment changes the answer


def pipe_with(dit=None, vae=None, dit2=None):
    from vstyler.pipeline import WanVideoPipeline
    pipe = WanVideoPipeline(device="cpu")
    pipe.dit, pipe.vae, pipe.dit2 = dit, vae, dit2
    return pipe


class FakeVae:
    def __init__(self, z_dim):
        self.z_dim = z_dim


def test_latent_geometry_and_division():
    ti2v = T.build(T.TINY_TI2V, None, device="meta")
    t2v = T.build(dict(T.TINY_TI2V, in_dim=16, out_dim=16), None, device="meta", fused=False)
    assert pipe_with().latent_geometry() == (16, 8)
    assert pipe_with(t2v).latent_geometry() == (16, 8)
    assert pipe_with(ti2v).latent_geometry() == (48, 16)
    assert pipe_with(ti2v, FakeVae(16)).latent_geometry() == (16, 8)      # the VAE's, when there is one
    assert pipe_with(t2v, FakeVae(48)).latent_geometry() == (48, 16)
    # a VAE of other latents: the DiT's can be produced (its geometry), not decoded
    mixed = pipe_with(ti2v, FakeVae(16))
    assert mixed.latent_geometry("latents") == (48, 16)
    assert mixed.check_resize_height_width(496, 848, output_type="latents") == (512, 864)
    with pytest.raises(RuntimeError, match='output_type="latents"'):
        mixed.latent_geometry("video")
    assert pipe_with(t2v).check_resize_height_width(470, 830, 80) == (480, 832, 81)      # unchanged
    assert pipe_with(ti2v).check_resize_height_width(470, 830, 80) == (480, 832, 81)
    assert pipe_with(ti2v).check_resize_height_width(704, 1280, 121) == (704, 1280, 121)
    assert pipe_with(ti2v).check_resize_height_width(496, 848) == (512, 864)             # multiples of 32
    assert pipe_with(t2v).check_resize_height_width(496, 848) == (496, 848)


def test_pipeline_argument_errors():
    ti2v = T.build(T.TINY_TI2V, None, device="meta")
    t2v = T.build(dict(T.TINY_TI2V, in_dim=16, out_dim=16), None, device="meta", fused=False)
    emb = torch.zeros(1, 8, 4096, dtype=BF16)
    ffl = torch.zeros(1, 48, 1, 4, 6, dtype=BF16)
    call = dict(prompt_emb=emb, negative_prompt_emb=emb, height=64, width=96, num_frames=5, num_inference_steps=2)
    with pytest.raises(ValueError, match="first_frame_latents"):
        pipe_with(t2v)(first_frame_latents=ffl, output_type="latents", **call)
    with pytest.raises(ValueError, match="first_frame_latents"):
        pipe_with(t2v).denoise(torch.zeros(1, 16, 2, 8, 12), emb, emb, first_frame_latents=ffl)
    with pytest.raises(NotImplementedError, match="first_frame_latents="):
        pipe_with(ti2v)(input_image=torch.zeros(64, 96, 3, dtype=torch.uint8), output_type="latents", **call)
    with pytest.raises(RuntimeError, match='output_type="latents"'):
        pipe_with(ti2v, FakeVae(16))(first_frame_latents=ffl, **call)
    with pytest.raises(ValueError, match="UniPC"):
        pipe_with(ti2v).denoise_unipc(torch.zeros(1, 48, 2, 4, 6), emb, emb, first_frame_latents=ffl)
    with pytest.raises(ValueError, match="enhance"):
        pipe_with(ti2v).enhance([], prompt_emb=emb, first_frame_latents=ffl)
    with pytest.raises(NotImplementedError, match="second expert"):
        pipe_with(ti2v, dit2=ti2v).denoise(torch.zeros(1, 48, 2, 4, 6), emb, emb, first_frame_latents=ffl)
    with pytest.raises(ValueError, match="expected"):
        pipe_with(ti2v).denoise(torch.zeros(1, 48, 2, 4, 6), emb, emb, first_frame_latents=ffl[:, :, :, :2])


def test_model_fn_refuses_what_the_segmented_path_lacks():
    from vstyler import model_fn_wan_video
    from vstyler.models import VaceWanModel
    ti2v = T.build(T.TINY_TI2V, None, device="meta")
    lat = torch.zeros(1, 48, 4, 4, 6, dtype=BF16)
    kw = dict(latents=lat, timestep=torch.tensor([500.0]), context=torch.zeros(2, 8, 4096, dtype=BF16),
              fuse_vae_embedding_in_latents=True)
    with pytest.raises(NotImplementedError, match="parallelism"):
        model_fn_wan_video(ti2v, use_unified_sequence_parallel=True, **kw)
    with pytest.raises(NotImplementedError, match="sliding window"):
        model_fn_wan_video(ti2v, sliding_window_size=2, sliding_window_stride=1, **kw)
    with pytest.raises(NotImplementedError, match="tea_cache"):
        model_fn_wan_video(ti2v, tea_cache=object(), **kw)
    vace = VaceWanModel(vace_layers=(0,), dim=256, num_heads=2, ffn_dim=512, device="meta")
    with pytest.raises(NotImplementedError, match="VACE"):
        model_fn_wan_video(ti2v, vace=vace, vace_context=torch.zeros(1, 96, 4, 4, 6, dtype=BF16), **kw)
    with pytest.raises(ValueError, match="one timestep"):
        model_fn_wan_video(ti2v, **dict(kw, timestep=torch.tensor([500.0, 400.0])))
