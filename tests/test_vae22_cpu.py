"""The Wan2.2 VAE (WanVideoVAE38) without a GPU: the whole-sequence restatement of tests/vae22_util.py against
the reference implementation's own chunked float64 run (tests/golden/vae22_ref.npz); the key layout against
the registry hash; the loader's choice of class; and the pipeline's input_image path on a
fuse_vae_embedding_in_latents DiT."""
import os

import numpy as np
import pytest
import torch

import ti2v_util as T
import vae22_util as U
from oracle import wan_vae_oracle as V

BF16 = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vae22_ref.npz")
SEED = 31                                    # tests/golden/make_vae22_ref.py
WAN22_VAE_HASH = "e1de6c02cdac79f8b739f4d3698cd216"


def _fixture_inputs():
    """The inputs of make_vae22_ref.py: bf16 values widened to float64."""
    g = torch.Generator().manual_seed(SEED)
    video = (torch.rand((1, 3, 9, 32, 48), generator=g) * 2 - 1).to(BF16).double()
    latent = torch.randn((1, 48, 3, 2, 3), generator=g).to(BF16).double()
    return video, latent


def test_restatement_equals_the_reference_in_float64():
    """max|d| <= 1e-9 max|ref|: float64 rounding over these depths stays below 1e-12, and a wrong frame
    pairing, channel order or a missing shortcut moves the output by more than 1e-2."""
    ref = np.load(GOLDEN)
    assert int(ref["seed"]) == SEED
    W = U.random_vae22_weights(U.TINY_VAE22, SEED)
    for key in [k for k in ref.files if k.startswith("abs_sum.")]:      # a drifted generator says so
        got = W[key[len("abs_sum."):]].double().abs().sum().item()
        assert got == float(ref[key]), f"the seeded weights changed ({key}): regenerate the fixture"
    video, latent = _fixture_inputs()
    for name, got in (("encode", U.encode_whole(video, W)), ("decode", U.decode_whole(latent, W))):
        want = torch.from_numpy(ref[name])
        assert got.dtype == torch.float64 and got.shape == want.shape
        d, scale = (got - want).abs().max().item(), want.abs().max().item()
        print(f"{name}: max|d| {d:.3g}, max|ref| {scale:.3g}")
        assert d <= 1e-9 * scale, (name, d, scale)


def test_key_layout_hash():
    from vstyler.loader import hash_state_dict_keys
    from vstyler.vae import WanVideoVAE38
    shapes = WanVideoVAE38(device="meta").state_dict_shapes()
    sd = {k: torch.empty(s, device="meta") for k, s in shapes.items()}
    assert len(sd) == 196 and sum(v.numel() for v in sd.values()) == 704688668
    assert hash_state_dict_keys(sd) == WAN22_VAE_HASH
    assert shapes == U.vae22_param_shapes(U.REAL_VAE22)
    tiny = WanVideoVAE38(dim=32, dec_dim=32, device="meta").state_dict_shapes()
    assert tiny == U.vae22_param_shapes(U.TINY_VAE22)


def test_loader_picks_the_class():
    from vstyler.loader import build_vae
    from vstyler.vae import WanVideoVAE, WanVideoVAE38
    meta = lambda shapes: {k: torch.empty(s, device="meta") for k, s in shapes.items()}  # noqa: E731
    m = build_vae(meta(U.vae22_param_shapes(U.TINY_VAE22)), "meta")
    assert type(m) is WanVideoVAE38
    assert (m.z_dim, m.dim, m.dec_dim, m.upsampling_factor) == (48, 32, 32, 16)
    assert set(m.cw) | set(m.params) >= {"model.encoder.downsamples.1.downsamples.2.time_conv.",
                                        "model.decoder.upsamples.0.upsamples.3.resample.1.",
                                        "model.decoder.head.0.gamma"}
    m = build_vae({"model_state": meta(U.vae22_param_shapes(U.TINY_VAE22))}, "meta")
    assert type(m) is WanVideoVAE38
    m = build_vae(meta(U.vae22_param_shapes(U.REAL_VAE22)), "meta")         # by the registry hash
    assert type(m) is WanVideoVAE38 and (m.dim, m.dec_dim) == (160, 256)
    m = build_vae(meta(V.vae_param_shapes(dict(V.VAE_CONFIG, dim=32))), "meta")
    assert type(m) is WanVideoVAE and m.z_dim == 16


class StubVae:
    """A VAE that records what it is asked to encode."""

    def __init__(self, z_dim, stride):
        self.z_dim, self.stride, self.calls = z_dim, stride, []

    def encode(self, videos, device=None, tiled=False, tile_size=None, tile_stride=None):
        self.calls.append(dict(videos=videos, tiled=tiled, tile_size=tile_size, tile_stride=tile_stride))
        v = videos[0]
        t = (v.shape[1] - 1) // 4 + 1
        return torch.full((len(videos), self.z_dim, t, v.shape[2] // self.stride, v.shape[3] // self.stride), 0.25,
                          dtype=BF16)


def _pipe(dit, vae):
    from vstyler.pipeline import WanVideoPipeline
    pipe = WanVideoPipeline(device="cpu")
    pipe.dit, pipe.vae = dit, vae
    return pipe


def test_pipeline_input_image_on_a_fused_dit(monkeypatch):
    from vstyler import vae as vae_mod
    ti2v = T.build(T.TINY_TI2V, None, device="meta")
    emb = torch.zeros(1, 8, 4096, dtype=BF16)
    call = dict(prompt_emb=emb, negative_prompt_emb=emb, height=64, width=96, num_frames=5, num_inference_steps=2,
                output_type="latents", tiled=True, tile_size=(2, 3), tile_stride=(1, 2))
    image = torch.arange(64 * 96 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(64, 96, 3)
    # without a 48-channel VAE: as before
    for vae in (None, StubVae(16, 8)):
        with pytest.raises(NotImplementedError, match="first_frame_latents="):
            _pipe(ti2v, vae)(input_image=image, **call)
    # with one: the preprocessed frame reaches encode, its result reaches denoise
    monkeypatch.setattr(vae_mod, "preprocess_video", V.preprocess_video)     # the CPU statement of the kernel
    seen = {}

    def denoise(latents, *args, **kw):
        seen.update(kw, latents=latents)
        return latents

    stub = StubVae(48, 16)
    pipe = _pipe(ti2v, stub)
    monkeypatch.setattr(pipe, "denoise", denoise)
    out = pipe(input_image=image, **call)
    assert tuple(out.shape) == (1, 48, 2, 4, 6)
    assert len(stub.calls) == 1
    c = stub.calls[0]
    assert (c["tiled"], tuple(c["tile_size"]), tuple(c["tile_stride"])) == (True, (2, 3), (1, 2))
    assert len(c["videos"]) == 1 and torch.equal(c["videos"][0], V.preprocess_video(image[None])[0])
    ffl = seen["first_frame_latents"]
    assert tuple(ffl.shape) == (1, 48, 1, 4, 6) and bool((ffl == 0.25).all())
    assert seen["y"] is None and seen["clip_feature"] is None
    # a PIL image is resized to the call's (width, height) first
    from PIL import Image
    big = Image.fromarray(np.asarray(image.repeat_interleave(2, 0).repeat_interleave(2, 1)))
    pipe(input_image=big, **call)
    want = torch.from_numpy(np.array(big.resize((96, 64))))
    assert torch.equal(stub.calls[1]["videos"][0], V.preprocess_video(want[None])[0])
    # an explicit first_frame_latents= wins: nothing is encoded
    mine = torch.full((1, 48, 1, 4, 6), -0.5, dtype=BF16)
    pipe(input_image=image, first_frame_latents=mine, **call)
    assert len(stub.calls) == 2 and torch.equal(seen["first_frame_latents"], mine)
