"""Wan2.2-TI2V-5B's image-to-video mode on the GPU: model_fn_wan_video(fuse_vae_embedding_in_latents=True) and
WanVideoPipeline.denoise(first_frame_latents=) on a tiny 48-channel DiT (latents 48 x 3 x 8 x 12: n0 = 24
tokens per latent frame, S = 72) against tests/ti2v_util.py, the literal per-token restatement, within the
oracle floor (the rule and constants of tests/test_i2v_gpu.py::within_floor: the float64 restatement
against the float32 one); and the bit-identities the two-row form must keep."""
import pytest
import torch

import ti2v_util as T
from gpu_util import err
from oracle import wan_oracle as O

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def within_floor(got, ref, ref64, tag):
    """tests/test_i2v_gpu.py::within_floor, unchanged."""
    fmx, frel = err(ref64, ref)
    mx, rel = err(got, ref)
    print(f"{tag}: max-abs {mx:.4g} rel-L2 {rel:.4g} (floor {fmx:.4g} / {frel:.4g})")
    assert rel <= 1.5 * frel + 2e-3 and mx <= 1.5 * fmx + 2e-2, (tag, mx, rel, fmx, frel)


@pytest.fixture(scope="module")
def model():
    cfg = T.TINY_TI2V
    W = T.random_weights(cfg)
    return cfg, W, T.build(cfg, W), T.inputs(cfg)


def fwd(dit, lat, t, ctx, fuse=True, **kw):
    from vstyler import model_fn_wan_video
    out = model_fn_wan_video(dit, latents=lat.cuda(), timestep=torch.tensor([t]).to(BF16).cuda(), context=ctx.cuda(),
                             fuse_vae_embedding_in_latents=fuse, **kw)
    torch.cuda.synchronize()
    return out.clone()


def test_forward_within_floor(model):
    cfg, W, dit, (lat, first, cp, cn) = model
    t = torch.tensor([637.0]).to(BF16)
    ctx = torch.cat([cp, cn])
    got = fwd(dit, lat, 637.0, ctx)
    assert got.shape == (2, 48, 3, 8, 12)

    def ref():
        return T.model_fn(W, cfg, lat, t, ctx)
    within_floor(got, ref(), T.with_float64(ref), "ti2v forward, CFG batch 2")
    # the segment matters: the plain forward of the same model is another function
    assert not torch.equal(bits(got), bits(fwd(dit, lat, 637.0, ctx, fuse=False)))


def test_t2v_on_the_same_model_within_floor(model):
    cfg, W, dit, (lat, first, cp, cn) = model
    t = torch.tensor([637.0]).to(BF16)
    got = fwd(dit, lat, 637.0, cp, fuse=False)

    def ref():
        return O.model_fn(W, cfg, lat, t, cp)
    within_floor(got, ref(), T.with_float64(ref), "t2v, 48 channels")


def test_bit_identities(model):
    from vstyler.options import host_options
    cfg, W, dit, (lat, first, cp, cn) = model
    ctx = torch.cat([cp, cn])
    # both rows at timestep 0: the plain forward at timestep 0
    assert torch.equal(bits(fwd(dit, lat, 0.0, ctx)), bits(fwd(dit, lat, 0.0, ctx, fuse=False)))
    # CFG batch 2 = two single forwards; the shared prefix on = off
    with host_options(cfg_prefix=1):
        on = fwd(dit, lat, 637.0, ctx)
    with host_options(cfg_prefix=0):
        off = fwd(dit, lat, 637.0, ctx)
    assert torch.equal(bits(on), bits(off))
    singles = torch.cat([fwd(dit, lat, 637.0, cp), fwd(dit, lat, 637.0, cn)])
    assert torch.equal(bits(on), bits(singles))
    # one latent frame: every token is the first frame's
    one = lat[:, :, :1].contiguous()
    assert torch.equal(bits(fwd(dit, one, 637.0, ctx)), bits(fwd(dit, one, 0.0, ctx, fuse=False)))
    # skip-layer guidance on the segmented path: sample 1 skips the block, sample 0 does not
    slg = fwd(dit, lat, 637.0, ctx, slg_blocks=(1,))
    assert torch.equal(bits(slg[0]), bits(on[0])) and not torch.equal(bits(slg[1]), bits(on[1]))


def test_persistent_route_size(model):
    """Latents 48 x 2 x 32 x 32: n0 = 256 >= 128, the segment lengths at which the gated GEMMs may stay on
    the 4-wave kernel if their shape reaches it.  Reference-free: both rows at timestep 0 is the plain
    forward; the float32 restatement bounds the rest."""
    cfg, W, dit, _ = model
    lat, first, cp, cn = T.inputs(cfg, T=2, h=32, w=32, seed=22)
    assert torch.equal(bits(fwd(dit, lat, 0.0, cp)), bits(fwd(dit, lat, 0.0, cp, fuse=False)))
    t = torch.tensor([500.0]).to(BF16)

    def ref():
        return T.model_fn(W, cfg, lat, t, cp)
    within_floor(fwd(dit, lat, 500.0, cp), ref(), T.with_float64(ref), "ti2v forward, n0 = 256")


def test_euler_loop_eager_graph_and_pin(model):
    from vstyler import WanVideoPipeline
    cfg, W, dit, (lat, first, cp, cn) = model
    pipe = WanVideoPipeline(device="cuda")
    pipe.dit = dit

    def run(**kw):
        return pipe.denoise(lat, cp.cuda(), cn.cuda(), num_inference_steps=2, first_frame_latents=first, **kw)
    eager = run(use_graph=False)
    assert pipe.last_graph is None
    graph = run(use_graph=True)
    assert pipe.last_graph is not None
    assert torch.equal(bits(eager), bits(graph))
    assert torch.equal(bits(graph[:, :, 0:1]), bits(first))

    def chain():
        return T.denoise(W, cfg, lat, first, cp, cn)
    within_floor(graph, chain(), T.with_float64(chain), "euler 2 steps, first_frame_latents")
    # through __call__ (output_type="latents"): the 48-channel noise shape, frame 0 pinned
    out = pipe(prompt_emb=cp, negative_prompt_emb=cn, height=128, width=192, num_frames=9, num_inference_steps=2,
               seed=3, first_frame_latents=first, output_type="latents")
    assert out.shape == (1, 48, 3, 8, 12) and torch.equal(bits(out[:, :, 0:1]), bits(first))


# --------------------------------------------------------------------- fp8 layers and hot-loaded LoRA
# The restatements: ti2v_util's blocks call O.blk_linear, so the oracle's own switches apply to the
# per-token path -- O.FP8_BLOCK_LINEARS with fp8_scaled_util's weight-scaled fp8_linear
# (quantize_fp8_(weight_scale="channel")), O.HOTLOAD with O.lora_linear (the un-merged adapter), and both
# (the adapter as the fp8 GEMM's bf16 second phase), the pattern of tests/test_fp8_scaled_model_gpu.py.
T_SEG = 637.0
LORA_TARGETS = ("blocks.0.self_attn.o", "blocks.0.ffn.0", "blocks.1.self_attn.q", "blocks.1.ffn.2")
LORA_ALPHA = 2.0


def make_lora(cfg, seed=9, r=32):
    g = torch.Generator().manual_seed(seed)
    D, F = cfg["dim"], cfg["ffn_dim"]
    lora = {}
    for name in LORA_TARGETS:
        out_f, in_f = {"ffn.0": (F, D), "ffn.2": (D, F)}.get(name.split(".", 2)[2], (D, D))
        lora[name + ".lora_A.default.weight"] = (0.05 * torch.randn(r, in_f, generator=g)).to(BF16)
        lora[name + ".lora_B.default.weight"] = (0.05 * torch.randn(out_f, r, generator=g)).to(BF16)
    return lora


def restate(monkeypatch, W, cfg, lat, ctx, fp8, lora):
    """(float32 restatement, float64 restatement) of the segmented forward at T_SEG with the oracle's fp8 /
    hot-load switches set for the duration of the test."""
    from fp8_scaled_util import fp8_linear_mode
    scaled = fp8_linear_mode("channel")
    if fp8:
        monkeypatch.setattr(O, "fp8_linear", scaled)
        monkeypatch.setattr(O, "FP8_BLOCK_LINEARS", True)
    if lora is not None:
        if fp8:         # layers.py:168-182: fp8_linear, then + x A^T B^T in bf16
            def lora_linear_fp8(x, w, b, lora_a, lora_b):
                tt = O.bf(x.float() @ lora_a.float().t())
                return O.bf(scaled(x, w, b).float() + O.bf(tt.float() @ lora_b.float().t()).float())
            monkeypatch.setattr(O, "lora_linear", lora_linear_fp8)
        for name in LORA_TARGETS:
            la, lb = (lora[f"{name}.lora_{x}.default.weight"] for x in "AB")
            monkeypatch.setitem(O.HOTLOAD, id(W[name + ".weight"]), (O.bf(la.float() * LORA_ALPHA), lb))
    t = torch.tensor([T_SEG]).to(BF16)

    def ref():
        return T.model_fn(W, cfg, lat, t, ctx)
    return ref(), T.with_float64(ref)


@pytest.mark.parametrize("variant", ["fp8", "lora", "fp8+lora"])
def test_fp8_layers_and_hot_lora_within_floor(monkeypatch, model, variant):
    """The segmented forward at a timestep where the two modulation rows differ, CFG batch 2, with fp8 block
    linears (the _fp8_seg LayerNorm into the fp8 GEMMs, their gated epilogue with seg_rows), with a
    hot-loaded LoRA (the gated GEMMs' second K phase) and with both, within the oracle floor of its
    restatement (within_floor, unchanged).

    fp8: as tests/test_fp8_scaled_model_gpu.py::test_model_fn_scaled_fp8_tiny_vs_oracle explains, the
    fp32-vs-fp64 floor of an fp8 forward is bimodal (no e4m3 rounding of an activation flips, or flips
    cascade through the blocks, rel-L2 >= 1e-3) while the GPU forward, which differs from the restatement
    by more than summation order, always sees flips; so, by that test's rule, the weights' seed is the
    first from 5 upwards whose floor is a cascade sample, chosen from the restatement alone before the GPU
    result is looked at.  On the 72-token latents the e4m3 GEMMs of this two-block model are exact in fp32
    (K = 256) and the floor of most seeds is 0 to 2e-4 -- no sample of that sensitivity --, so the fp8
    variants run at the 512-token size, where the restatement does show cascades."""
    from vstyler.lora import hotload_lora
    from vstyler.models import quantize_fp8_
    cfg, W5, _, (lat, first, cp, cn) = model
    ctx = torch.cat([cp, cn])
    fp8, lora = "fp8" in variant, make_lora(cfg) if "lora" in variant else None
    if fp8:         # the issue's second size, 48 x 2 x 32 x 32 (n0 = 256): see the docstring
        lat, first, cp, cn = T.inputs(cfg, T=2, h=32, w=32, seed=22)
        ctx = torch.cat([cp, cn])
    for seed in range(5, 13):
        W = W5 if seed == 5 else T.random_weights(cfg, seed=seed)
        ref, ref64 = restate(monkeypatch, W, cfg, lat, ctx, fp8, lora)
        fmx, frl = err(ref64, ref)
        print(f"{variant} seed {seed}: restatement fp32-vs-fp64 floor max-abs {fmx:.4g} rel-L2 {frl:.4g}")
        if not fp8 or frl >= 1e-3:
            break
    else:
        pytest.fail("no seed with a cascade sample of the floor")
    dit = T.build(cfg, W)
    if fp8:
        assert quantize_fp8_(dit, weight_scale="channel") == 10 * cfg["num_layers"]
    bare = fwd(dit, lat, T_SEG, ctx)
    if lora is not None:
        assert hotload_lora(dit, lora, LORA_ALPHA, **(dict(fp8_layers="fuse") if fp8 else {})) == len(LORA_TARGETS)
    got = fwd(dit, lat, T_SEG, ctx)
    within_floor(got, ref, ref64, f"ti2v segmented forward, {variant} (seed {seed})")
    # the segment and the adapter both matter; with both rows at timestep 0 the path is the plain one's
    assert not torch.equal(bits(got), bits(fwd(dit, lat, T_SEG, ctx, fuse=False)))
    if lora is not None:
        assert not torch.equal(bits(got), bits(bare))
    assert torch.equal(bits(fwd(dit, lat, 0.0, ctx)), bits(fwd(dit, lat, 0.0, ctx, fuse=False)))
