"""GPU parity of the Wan2.2 VAE (vstyler.vae.WanVideoVAE38) against the whole-sequence restatement of
tests/vae22_util.py -- itself held to the reference implementation's chunked run by tests/test_vae22_cpu.py --
under the rule of tests/test_vae_gpu.py: within 1.5x the restatement's own fp32-vs-fp64 accumulation floor plus
1e-3 rel-L2 / 1e-2 max-abs.  The tiny configuration end to end (untiled and tiled), one Down and one Up block
at the real widths, and the TI2V pipeline's image, video and decode paths through the tiny model."""
import pytest
import torch

import ti2v_util as T
import vae22_util as U22
from gpu_util import err
from oracle import wan_oracle as O
from vae_util import synthetic_video

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
TILE, STRIDE = (2, 3), (1, 2)


def bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.uint8)


def _floor(fn):
    """(fp32-accumulation result, its distance from the fp64-accumulation one): test_vae_gpu.py::_floor."""
    old = O.ACC_DTYPE
    try:
        O.ACC_DTYPE = torch.float64
        r64 = fn()
    finally:
        O.ACC_DTYPE = old
    r32 = fn()
    return r32, err(r64, r32)


def _within_floor(got, ref, floor, tag):
    mx, rel = err(got, ref)
    fmx, frel = floor
    print(f"{tag}: max-abs {mx:.4g} rel-L2 {rel:.4g} (floor {fmx:.4g} / {frel:.4g})")
    assert rel <= 1.5 * frel + 1e-3 and mx <= 1.5 * fmx + 1e-2, dict(tag=tag, gpu=(mx, rel), floor=floor)


def _model(cfg, W):
    from vstyler import vae
    m = vae.WanVideoVAE38(z_dim=cfg["z_dim"], dim=cfg["dim"], dec_dim=cfg["dec_dim"], dim_mult=cfg["dim_mult"],
                          num_res_blocks=cfg["num_res_blocks"], temperal_downsample=cfg["temperal_downsample"],
                          device="cuda")
    return m.load_state_dict(W)


@pytest.fixture(scope="module")
def tiny():
    W = U22.random_vae22_weights(U22.TINY_VAE22, seed=41)
    return W, _model(U22.TINY_VAE22, W)


@pytest.mark.parametrize("tiled", [False, True])
def test_encode_tiny(tiny, tiled):
    W, m = tiny
    video = synthetic_video(9, 64, 96)
    if tiled:
        ref, floor = _floor(lambda: U22.tiled_encode(video, W, TILE, STRIDE))
    else:
        ref, floor = _floor(lambda: U22.encode_whole(video, W))
    got = m.encode(video.cuda(), "cuda", tiled=tiled, tile_size=TILE, tile_stride=STRIDE)
    assert got.shape == ref.shape == (1, 48, 3, 4, 6)
    _within_floor(got, ref, floor, f"encode tiny, tiled={tiled}")


@pytest.mark.parametrize("tiled", [False, True])
def test_decode_tiny(tiny, tiled):
    """Measured on an MI355X (16 CPU threads for the restatement): untiled rel-L2 0.01308 against a floor of
    0.01109 (bar 0.01763), tiled 0.01062 against 0.00813 (bar 0.01320).  The case is sensitive: the DupUp3D
    shortcuts carry the decoder's middle block to every level, and with the attention probabilities rounded
    to bf16 before P.V, as WanVideoVAE's routes round them, the tiled decode sat at 0.01354 -- that rounding
    alone, applied to the CPU restatement, moves it by 0.0135.  WanVideoVAE38._attn_block therefore keeps P as a
    bf16 hi / lo pair (vs_vae22_softmax_split)."""
    W, m = tiny
    z = torch.randn((1, 48, 3, 4, 6), generator=torch.Generator().manual_seed(4)).to(BF16)
    if tiled:
        ref, floor = _floor(lambda: U22.tiled_decode(z, W, TILE, STRIDE))
    else:
        ref, floor = _floor(lambda: U22.single_decode(z, W))
    got = m.decode(z.cuda(), "cuda", tiled=tiled, tile_size=TILE, tile_stride=STRIDE)
    assert got.shape == ref.shape == (1, 3, 9, 64, 96)
    _within_floor(got, ref, floor, f"decode tiny, tiled={tiled}")


@pytest.mark.parametrize("part,index,c_in", [("encoder", 1, 160), ("decoder", 1, 1024)])
def test_block_at_real_widths(part, index, c_in):
    """The second Down block (160 -> 320, temporal and spatial AvgDown3D) and the second Up block (1024 -> 512,
    temporal and spatial DupUp3D) of the real configuration alone, on a (1, C, 3, 4, 6) input."""
    from vstyler import vae
    cfg = U22.REAL_VAE22
    layers, sc = U22.blocks(cfg, part)[0][index]
    assert sc[0] == c_in and sc[2:] == (2, 2)
    g = torch.Generator().manual_seed(c_in)
    prefixes = tuple(p for _, p, _ in layers)
    W = U22.random_vae22_weights(cfg, seed=43, prefixes=prefixes)
    x = torch.randn((1, c_in, 3, 4, 6), generator=g).to(BF16)
    ref, floor = _floor(lambda: U22.run_block(x, W, layers, sc, part))
    m = vae.WanVideoVAE38(device="cuda").load_state_dict(W)
    blocks = (m.enc_layers if part == "encoder" else m.dec_layers)[index:index + 1]
    add = vae.avgdown_add if part == "encoder" else vae.dupup_add
    got = m._run_blocks(x.permute(0, 2, 3, 4, 1).contiguous().cuda(), blocks, add).cpu().permute(0, 4, 1, 2, 3)
    assert got.shape == ref.shape
    _within_floor(got, ref, floor, f"{part} block {index} at real widths")


@pytest.fixture(scope="module")
def pipe(tiny):
    from vstyler.pipeline import WanVideoPipeline
    cfg = T.TINY_TI2V
    p = WanVideoPipeline(device="cuda")
    p.dit = T.build(cfg, T.random_weights(cfg))
    p.vae = tiny[1]
    _, _, cp, cn = T.inputs(cfg)
    call = dict(prompt_emb=cp, negative_prompt_emb=cn, height=128, width=192, num_frames=9, num_inference_steps=2,
                seed=3, tiled=True, tile_size=(4, 6), tile_stride=(2, 3))
    return p, call


def test_pipeline_input_image_is_first_frame_latents(pipe):
    from vstyler.vae import frames_to_u8, preprocess_video
    p, call = pipe
    image = torch.randint(0, 256, (128, 192, 3), generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
    got = p(input_image=image, output_type="latents", **call)
    frame = preprocess_video(frames_to_u8(image[None], "cuda"))
    first = p.vae.encode([frame[0]], "cuda", tiled=True, tile_size=(4, 6), tile_stride=(2, 3))
    assert first.shape == (1, 48, 1, 8, 12)
    want = p(first_frame_latents=first, output_type="latents", **call)
    assert got.shape == (1, 48, 3, 8, 12)
    assert torch.equal(bits(got), bits(want)) and torch.equal(bits(got[:, :, 0:1]), bits(first))


def test_pipeline_decodes_video(pipe):
    from vstyler.vae import vae_output_to_u8
    p, call = pipe
    first = torch.randn((1, 48, 1, 8, 12), generator=torch.Generator().manual_seed(9)).to(BF16).cuda()
    latents = p(first_frame_latents=first, output_type="latents", **call)
    frames = p(first_frame_latents=first, output_type="u8", **call)
    video = p.vae.decode(latents, "cuda", tiled=True, tile_size=(4, 6), tile_stride=(2, 3))
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (9, 128, 192, 3)
    assert torch.equal(bits(frames), bits(vae_output_to_u8(video[0])))
    pil = p(first_frame_latents=first, output_type="video", **call)
    assert len(pil) == 9 and pil[0].size == (192, 128)
    import numpy as np
    assert all(np.array_equal(np.asarray(f), frames[i].cpu().numpy()) for i, f in enumerate(pil))


def test_pipeline_input_video_is_input_latents(pipe):
    from vstyler.vae import preprocess_video
    p, call = pipe
    video = torch.randint(0, 256, (9, 128, 192, 3), generator=torch.Generator().manual_seed(10), dtype=torch.uint8)
    got = p(input_video=video, denoising_strength=0.6, output_type="latents", **call)
    lat = p.vae.encode(preprocess_video(video.cuda()), "cuda", tiled=True, tile_size=(4, 6), tile_stride=(2, 3))
    assert lat.shape == (1, 48, 3, 8, 12)
    want = p(input_latents=lat, denoising_strength=0.6, output_type="latents", **call)
    assert torch.equal(bits(got), bits(want))
