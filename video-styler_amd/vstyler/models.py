"""Wan2.1 DiT + VACE branch on MI355X.

Parameter containers keep the reference's module names and shapes (so a reference state dict
loads by name and reproduces the reference's md5 key-layout hash, models/utils.py:148-182); the
forward passes are sequences of libvstyler kernels (vstyler.kernels), never torch math.

Reference: diffsynth/models/wan_video_dit.py (DiTBlock :196-230, Head :253-269, WanModel
:272-352), diffsynth/models/wan_video_vace.py (:5-87), model_fn_wan_video
(diffsynth/pipelines/wan_video_new.py:1260-1468).
"""
import math

import torch
import torch.nn as nn

from . import kernels as K
from .options import host_option

BF16 = torch.bfloat16


def _param(*shape, device=None, dtype=BF16):
    return nn.Parameter(torch.empty(*shape, device=device, dtype=dtype), requires_grad=False)


class Linear(nn.Module):
    """Weight [out, in] + bias, bf16 (the nn.Linear layout the MFMA GEMM reads K-contiguous)."""

    def __init__(self, in_features, out_features, bias=True, device=None, dtype=BF16):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = _param(out_features, in_features, device=device, dtype=dtype)
        self.bias = _param(out_features, device=device, dtype=dtype) if bias else None


class Q8:
    """An activation already quantised for fp8_linear (x8 e4m3 bytes [M, K], per-row scale [M]): what
    ln_into() hands to linear() / fused_linear() when the consumer is an fp8 layer."""

    def __init__(self, x8, scale):
        self.x8, self.scale = x8, scale
        self.shape = x8.shape


def _fp8_consumer(target):
    """True when `target` (a Linear, or a module whose fused projections run as one GEMM) consumes
    its input through fp8_linear."""
    if isinstance(target, AttentionParams):
        f = _fused_views(target)
        return f is not None and f[2] is not None
    return getattr(target, "weight_fp8", None) is not None and getattr(target, "lora_A", None) is None


def ln_into(x, h, ws, target, eps, **ln):
    """LayerNorm(+modulate) of x for `target`'s projection: into the bf16 buffer h, or -- when target
    runs fp8_linear -- straight into its quantised activation (vs_layernorm_modulate_fp8: the bf16 row
    is never stored and not re-read; bit-identical)."""
    seg = ln.pop("seg_rows", 0)     # two modulation rows per sample (RunCtx.seg_rows): the _seg entries
    if target is not None and _fp8_consumer(target):
        M, D = x.shape
        x8, qs = ws.get("fp8_x", (M, D), torch.uint8), ws.get("fp8_scale", (M,), torch.float32)
        if seg:
            return Q8(*K.layernorm_modulate_fp8_seg(x, x8, qs, seg, eps, **ln))
        return Q8(*K.layernorm_modulate_fp8(x, x8, qs, eps, **ln))
    if seg:
        K.layernorm_modulate_seg(x, h, seg, eps, **ln)
    else:
        K.layernorm_modulate(x, h, eps, **ln)
    return h


def linear(lin, x, out, ws, **epi):
    """Linear through vs_gemm; a hot-loaded LoRA (lin.lora_A = alpha*A, lin.lora_B = B) is fused as
    the GEMM's second K phase (AutoWrappedLinear, vram_management/layers.py:173-188).  A layer
    converted by quantize_fp8_ runs the fp8 path of AutoWrappedLinear.fp8_linear (:115-151):
    per-row activation quantisation (or the Q8 input ln_into made) + e4m3 MFMA GEMM with the same
    fused epilogue.  A LoRA hot-loaded onto an fp8 layer (hotload_lora(fp8_layers="fuse")) is the fp8
    GEMM's bf16 second K phase (layers.py:168-182: fp8_linear, then + x A^T B^T): its down-projection
    reads the bf16 row, so such a layer takes no Q8 input (ln_into hands it bf16 rows).  A layer with a
    weight_scale (fp32 [N]: W = weight_scale[n] * weight_fp8[n]) hands it to the GEMM on all three forms."""
    w8 = getattr(lin, "weight_fp8", None)
    if w8 is not None:
        la = getattr(lin, "lora_A", None)
        if getattr(lin, "weight_scale", None) is not None:      # quantize_fp8_(weight_scale=...) / a scaled checkpoint
            epi = dict(epi, scale_w=lin.weight_scale)
        if isinstance(x, Q8):
            if la is not None:
                raise ValueError("a quantised activation for an fp8 layer with a hot-loaded LoRA")
            return K.gemm_fp8(x.x8, x.scale, w8, out, bias=lin.bias, **epi)
        M, Kd = x.shape
        x8 = ws.get("fp8_x", (M, Kd), torch.uint8)
        sc = ws.get("fp8_scale", (M,), torch.float32)
        K.quant_fp8_rows(x, x8, sc)
        if la is not None:
            t = ws.get("lora_t", (M, la.shape[0]))
            K.gemm(x, la, t)
            return K.gemm_fp8(x8, sc, w8, out, bias=lin.bias, a2=t, w2=lin.lora_B, **epi)
        return K.gemm_fp8(x8, sc, w8, out, bias=lin.bias, **epi)
    if isinstance(x, Q8):
        raise ValueError("a quantised activation for a bf16 layer")
    la = getattr(lin, "lora_A", None)
    a2 = w2 = None
    if la is not None:
        t = ws.get("lora_t", (x.shape[0], la.shape[0]))
        K.gemm(x, la, t)
        a2, w2 = t, lin.lora_B
    return K.gemm(x, lin.weight, out, bias=lin.bias, a2=a2, w2=w2, **epi)


FP8_WEIGHT_SCALE_MODES = ("channel", "tensor")


def fp8_weight_scale(weight, mode):
    """The fp32 [N] scale of a Linear's weight [N, K] for its e4m3 copy: "channel": sw[n] =
    max_k |W[n][k]| / 448 (448 = the largest e4m3fn value), "tensor": max |W| / 448 broadcast to [N];
    an all-zero row (tensor) gets 1.  The N quotients are formed on the host: a device tensor divided
    by a Python scalar is multiplied by the scalar's rounded reciprocal there, which is not the fp32
    quotient in every case."""
    if mode not in FP8_WEIGHT_SCALE_MODES:
        raise ValueError(f"weight_scale must be None, 'channel' or 'tensor', got {mode!r}")
    a = weight.detach().float().abs()
    amax = (a.amax(dim=1) if mode == "channel" else a.amax().expand(a.shape[0])).cpu()
    sw = torch.where(amax == 0, torch.ones_like(amax), amax / torch.full_like(amax, 448.0))
    return sw.contiguous().to(weight.device)


def fp8_quantize_weight(weight, scale):
    """e4m3fn(W.float() / sw[n]) as uint8 bytes."""
    return (weight.detach().float() / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)


def block_fp8_linears(blk):
    """The Linears of a DiT / VACE block that quantize_fp8_ converts."""
    return (blk.self_attn.q, blk.self_attn.k, blk.self_attn.v, blk.self_attn.o, blk.cross_attn.q,
            blk.cross_attn.k, blk.cross_attn.v, blk.cross_attn.o, blk.ffn[0], blk.ffn[2])


def quantize_fp8_(module, weight_scale=None):
    """Give every block Linear (self/cross-attention q/k/v/o, FFN; DiT and VACE blocks) an e4m3fn
    copy of its weight used by linear(); embeddings, VACE before/after projections and the head stay
    bf16.  weight_scale None: the raw cast weight.to(float8_e4m3fn), as fp8_linear casts it
    (layers.py:133, scale_b = 1).  "channel" / "tensor": the copy is e4m3fn(W / sw[n]) with
    fp8_weight_scale's per-output-channel / per-Linear scale, which the GEMM multiplies back in fp32
    (the scale_b operand of torch._scaled_mm): each Linear gets weight_scale (fp32 [N]) and
    weight_scale_mode, the fused q|k|v / k|v buffers one fused scale vector the per-Linear scales are
    views of."""
    if weight_scale is not None and weight_scale not in FP8_WEIGHT_SCALE_MODES:
        raise ValueError(f"weight_scale must be None, 'channel' or 'tensor', got {weight_scale!r}")
    n = 0
    for blk in [m for m in module.modules() if isinstance(m, DiTBlock)]:
        for lin in block_fp8_linears(blk):      # (a re-conversion: the fused check below sees bf16 layers)
            for a in ("weight_fp8", "weight_scale", "weight_scale_mode"):
                if hasattr(lin, a):
                    delattr(lin, a)
        for att in (blk.self_attn, blk.cross_attn):
            att._fw8 = att._fsw = None
            if _fused_views(att) is not None:       # fused q|k|v / k|v: one e4m3 buffer, per-Linear views
                if weight_scale is None:
                    att._fw8 = att._fw.to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
                else:
                    att._fw8 = torch.empty(att._fw.shape, dtype=torch.uint8, device=att._fw.device)
                    att._fsw = torch.empty(att._fw.shape[0], dtype=torch.float32, device=att._fw.device)
        for lin in block_fp8_linears(blk):
            if weight_scale is None:
                lin.weight_fp8 = lin.weight.detach().to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
            else:
                lin.weight_scale = fp8_weight_scale(lin.weight, weight_scale)
                lin.weight_scale_mode = weight_scale
                lin.weight_fp8 = fp8_quantize_weight(lin.weight, lin.weight_scale).contiguous()
            n += 1
        for att in (blk.self_attn, blk.cross_attn):
            if att._fw8 is not None:
                d = att.dim
                for i, name in enumerate(att.fused):
                    lin = getattr(att, name)
                    if weight_scale is not None:
                        att._fw8[i * d:(i + 1) * d].copy_(lin.weight_fp8)
                        att._fsw[i * d:(i + 1) * d].copy_(lin.weight_scale)
                        lin.weight_scale = att._fsw[i * d:(i + 1) * d]
                    lin.weight_fp8 = att._fw8[i * d:(i + 1) * d]
    return n


class PatchEmbed(nn.Module):
    """Conv3d(in, dim, k=s=(1,2,2)) parameters (wan_video_dit.py:306-307)."""

    def __init__(self, in_dim, dim, device=None):
        super().__init__()
        self.in_dim, self.dim = in_dim, dim
        self.weight = _param(dim, in_dim, 1, 2, 2, device=device)
        self.bias = _param(dim, device=device)
        self._wpad = self._wpad_of = None

    def padded_weight(self):
        """The weight as [dim, Kp], Kp = 4 in_dim rounded up to the GEMM's K step of 64, the columns past
        4 in_dim zero (vs_patchify2 zero-fills the same columns of the token rows: 36 channels give
        K = 144 in 192).  Built once per loaded weight (rebuilt when the parameter is written again)."""
        key = (self.weight.data_ptr(), self.weight._version)
        if self._wpad is None or self._wpad_of != key:
            k = 4 * self.in_dim
            wp = torch.zeros((self.dim, (k + 63) // 64 * 64), device=self.weight.device, dtype=BF16)
            wp[:, :k].copy_(self.weight.detach().reshape(self.dim, k))
            self._wpad, self._wpad_of = wp, key
        return self._wpad

    def forward(self, lat, ws, tag, y=None, batch=None, skip=0, residual=None):
        """lat [B, C, T, H, W] -> tokens [B*S, dim].  y [B or 1, in_dim - C, T, H, W]: the channels
        concatenated behind lat's (wan_video_new.py:1367-1368), read in place by vs_patchify2; with y
        (or with 4 in_dim no multiple of 64) the token rows and the weight are K-padded.  batch: the
        output samples when lat and y are batch-1 operands broadcast over the CFG batch.

        residual [B*S, dim]: added in the GEMM's epilogue, bf16(residual + bf16(acc + bias)) (the camera
        adapter's output, wan_video_dit.py:341-344).  skip > 0: the output is [B*(skip + S), dim] and sample
        b's tokens are its rows skip.. (the rows in front are the caller's: the reference image's tokens),
        written by one GEMM per sample through a row view."""
        B, C, T, H, W = lat.shape
        S = T * (H // 2) * (W // 2)
        epi = {} if residual is None else dict(epilogue=K.VS_EPI_RES, residual=residual)
        if y is None and batch is None and (C * 4) % 64 == 0:
            cols = ws.get(tag + ".cols", (B * S, C * 4))
            K.patchify(lat.contiguous(), cols)
            w = self.weight.view(self.dim, C * 4)
        else:
            B = B if batch is None else batch
            w = self.padded_weight()
            cols = ws.get(tag + ".cols", (B * S, w.shape[1]))
            K.patchify2(lat.contiguous(), None if y is None else y.contiguous(), cols)
        if not skip:
            out = ws.get(tag + ".out", (B * S, self.dim))
            K.gemm(cols, w, out, bias=self.bias, **epi)
            return out, (T, H // 2, W // 2)
        R = skip + S
        out = ws.get(tag + ".out", (B * R, self.dim))
        for b in range(B):
            if residual is not None:
                epi["residual"] = residual[b * S:(b + 1) * S]
            K.gemm(cols[b * S:(b + 1) * S], w, out[b * R + skip:(b + 1) * R], bias=self.bias, **epi)
        return out, (T, H // 2, W // 2)


class RMSNormW(nn.Module):
    def __init__(self, dim, device=None):
        super().__init__()
        self.weight = _param(dim, device=device)


class LayerNormAffine(nn.Module):
    def __init__(self, dim, device=None):
        super().__init__()
        self.weight = _param(dim, device=device)
        self.bias = _param(dim, device=device)


class AttentionParams(nn.Module):
    """q/k/v/o Linears + QK norms under the reference's key names.  The Linears listed in `fused`
    (same input: q|k|v of self-attention, k|v of cross-attention) keep their weights and biases as
    row slices of one [n*dim, dim] / [n*dim] buffer, so their projections run as ONE GEMM
    (fused_linear); state-dict loading, LoRA merging and init all write through the slices."""

    def __init__(self, dim, num_heads, device=None, fused=(), image=False):
        super().__init__()
        self.dim, self.num_heads = dim, num_heads
        self.q = Linear(dim, dim, device=device)
        self.k = Linear(dim, dim, device=device)
        self.v = Linear(dim, dim, device=device)
        self.o = Linear(dim, dim, device=device)
        self.norm_q = RMSNormW(dim, device=device)
        self.norm_k = RMSNormW(dim, device=device)
        self.fused = tuple(fused)
        self._fw = self._fb = self._fw8 = self._fsw = None
        if self.fused:
            n = len(self.fused)
            self._fw = torch.empty(n * dim, dim, device=device, dtype=BF16)
            self._fb = torch.empty(n * dim, device=device, dtype=BF16)
            for i, name in enumerate(self.fused):
                lin = getattr(self, name)
                lin.weight = nn.Parameter(self._fw[i * dim:(i + 1) * dim], requires_grad=False)
                lin.bias = nn.Parameter(self._fb[i * dim:(i + 1) * dim], requires_grad=False)
        # the image branch of CrossAttention (wan_video_dit.py:164-167): k_img | v_img fused like k | v
        self.has_image_input = bool(image)
        if image:
            self.k_img = Linear(dim, dim, device=device)
            self.v_img = Linear(dim, dim, device=device)
            self.norm_k_img = RMSNormW(dim, device=device)
            self._fw_img = torch.empty(2 * dim, dim, device=device, dtype=BF16)
            self._fb_img = torch.empty(2 * dim, device=device, dtype=BF16)
            for i, lin in enumerate((self.k_img, self.v_img)):
                lin.weight = nn.Parameter(self._fw_img[i * dim:(i + 1) * dim], requires_grad=False)
                lin.bias = nn.Parameter(self._fb_img[i * dim:(i + 1) * dim], requires_grad=False)


def _fused_views(mod):
    """(W, b, W8 or None) when the fused Linears still alias the fused buffers (nothing rebound
    their parameters, no hot-loaded LoRA, fp8 copies all present or all absent, their weight scales
    all absent or all views of the fused scale vector: _fused_scale), else None."""
    if not getattr(mod, "fused", ()) or mod._fw is None:
        return None
    d = mod.dim
    fp8 = [getattr(getattr(mod, n), "weight_fp8", None) is not None for n in mod.fused]
    if any(fp8) and (not all(fp8) or mod._fw8 is None):
        return None
    sc = [getattr(getattr(mod, n), "weight_scale", None) for n in mod.fused]
    if any(s is not None for s in sc):
        fsw = getattr(mod, "_fsw", None)
        if not all(fp8) or fsw is None or any(s is None for s in sc):
            return None
        for i, s in enumerate(sc):
            if s.data_ptr() != fsw[i * d:].data_ptr() or s.shape != (d,) or s.stride(0) != 1:
                return None
    for i, name in enumerate(mod.fused):
        lin = getattr(mod, name)
        if getattr(lin, "lora_A", None) is not None:
            return None
        if lin.weight.data_ptr() != mod._fw[i * d].data_ptr() or lin.bias is None or \
                lin.bias.data_ptr() != mod._fb[i * d:].data_ptr():
            return None
        if fp8[i] and lin.weight_fp8.data_ptr() != mod._fw8[i * d].data_ptr():
            return None
    return mod._fw, mod._fb, (mod._fw8 if all(fp8) else None)


def _fused_scale(mod):
    """The fused weight-scale vector [n*dim] of a module whose fused Linears carry scales (checked
    by _fused_views), else None."""
    if getattr(getattr(mod, mod.fused[0]), "weight_scale", None) is None:
        return None
    return mod._fsw


def fused_linear(mod, x, ws, tag):
    """All of mod.fused's projections of x as one GEMM into a [M, n*dim] buffer (column block i =
    Linear i), or None when the fusion does not apply (the caller runs them one by one)."""
    f = _fused_views(mod)
    if f is None:
        return None
    W, b, W8 = f
    out = ws.get("fused" + tag, (x.shape[0], W.shape[0]))
    sw = {} if W8 is None or _fused_scale(mod) is None else {"scale_w": mod._fsw}
    if W8 is not None and isinstance(x, Q8):
        return K.gemm_fp8(x.x8, x.scale, W8, out, bias=b, **sw)
    if W8 is not None:
        M, Kd = x.shape
        x8 = ws.get("fp8_x", (M, Kd), torch.uint8)
        sc = ws.get("fp8_scale", (M,), torch.float32)
        K.quant_fp8_rows(x, x8, sc)
        return K.gemm_fp8(x8, sc, W8, out, bias=b, **sw)
    return K.gemm(x, W, out, bias=b)


def fused_img_linear(mod, x, ws, tag):
    """k_img | v_img of the image rows x as one bf16 GEMM into [M, 2 dim], or None when the two no
    longer alias the fused buffer or carry a hot-loaded LoRA (the caller runs them one by one).  The
    image projections stay bf16: quantize_fp8_ does not convert them."""
    d = mod.dim
    for i, lin in enumerate((mod.k_img, mod.v_img)):
        if getattr(lin, "lora_A", None) is not None or getattr(lin, "weight_fp8", None) is not None:
            return None
        if lin.weight.data_ptr() != mod._fw_img[i * d].data_ptr() or lin.bias is None or \
                lin.bias.data_ptr() != mod._fb_img[i * d:].data_ptr():
            return None
    return K.gemm(x, mod._fw_img, ws.get("fused" + tag, (x.shape[0], 2 * d)), bias=mod._fb_img)


class Sequential3(nn.Module):
    """Holds modules at indices 0 and 2 (Linear, act, Linear) to keep the reference's key names."""

    def __init__(self, first, last):
        super().__init__()
        self.add_module("0", first)
        self.add_module("2", last)

    def __getitem__(self, i):
        return getattr(self, str(i))


class Workspace:
    """Scratch buffers reused across blocks/steps (kernels never allocate).  A buffer is keyed by
    (name, shape, dtype) and lives as long as the workspace: forwards of different sizes that alternate
    -- the full and the ragged window of a sliding-window step -- each keep their own set, so after one
    forward at every size nothing is allocated and no buffer moves (a captured step stays valid)."""

    def __init__(self, device):
        self.device = device
        self.bufs = {}

    def get(self, name, shape, dtype=BF16):
        key = (name, tuple(int(s) for s in shape), dtype)
        t = self.bufs.get(key)
        if t is None:
            t = torch.empty(key[1], device=self.device, dtype=dtype)
            if host_option("ws_poison"):    # debugging aid: NaN-fill so a read-before-write shows up
                t.view(torch.uint8).fill_(0xFF)
            self.bufs[key] = t
        return t


class KernelTimer:
    """Optional HIP-event bracketing of chosen launches (bench.py roofline): events are recorded on
    the stream the kernel is launched on (torch's current stream), elapsed times read afterwards.
    Inactive while a hipGraph is being captured (ROCm refuses external event nodes in graphs)."""

    def __init__(self):
        self.enabled = False
        self.events = {}

    def start(self, name, flops=0.0):
        """flops: the launch's algorithmic FLOPs (tflops() divides their sum by the summed time)."""
        if not self.enabled or torch.cuda.is_current_stream_capturing():
            return None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.events.setdefault(name, []).append((e0, e1, float(flops)))
        return e1

    def stop(self, e1):
        if e1 is not None:
            e1.record()

    def mean_ms(self, name):
        ev = self.events.get(name, [])
        if not ev:
            return None, 0
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b, _ in ev) / len(ev), len(ev)

    def tflops(self, name):
        """Summed FLOPs / summed launch time of the bracketed launches (TFLOP/s), or None."""
        ev = self.events.get(name, [])
        if not ev:
            return None
        torch.cuda.synchronize()
        ms = sum(a.elapsed_time(b) for a, b, _ in ev)
        return sum(f for _, _, f in ev) / (ms / 1000.0) / 1e12 if ms > 0 else None

    def reset(self):
        self.events = {}


TIMER = KernelTimer()


def attn_flops(q, k, batch):
    """4 Sq Skv (heads x d) per sample: QK^T and PV of one attention launch (q: [batch Sq, heads d])."""
    return 4.0 * (q.shape[0] // batch) * (k.shape[0] // batch) * q.shape[1] * batch


IMG_TOKENS = 257      # CLIP ViT-H/14 tokens of one image: the rows CrossAttention splits off (:172-174)


class RunCtx:
    """Per-forward constants shared by all blocks: batch/token geometry, RoPE table, SP info."""

    def __init__(self, batch, seq, grid, rope, ctx, ctx_len, ws, sp=None, token_offset=0):
        self.batch, self.seq, self.grid, self.rope = batch, seq, grid, rope
        self.ctx, self.ctx_len, self.ws = ctx, ctx_len, ws
        self.sp = sp                    # vstyler.usp.UlyssesGroup or None
        self.token_offset = token_offset
        # image conditioning: the embedded CLIP rows every block's image cross-attention reads,
        # [img_batch * IMG_TOKENS, D] (img_batch 1: one key set shared by every CFG sample), or None
        self.img, self.img_batch = None, 0
        # two modulation rows per sample (a fused-first-frame DiT, model_fn_wan_video): the first
        # seg_rows token rows of every sample read modulation row 2 b, the rest 2 b + 1; 0: one row
        self.seg_rows = 0

    @property
    def seg(self):
        """The seg_rows= keyword of the modulated LayerNorms and the gated GEMMs (none when unsegmented)."""
        return {"seg_rows": self.seg_rows} if self.seg_rows else {}


class DiTBlock(nn.Module):
    """wan_video_dit.py:196-230 parameters; forward = fused kernel sequence on [B*S, D] rows."""

    def __init__(self, dim, num_heads, ffn_dim, eps=1e-6, device=None, has_image_input=False):
        super().__init__()
        self.dim, self.num_heads, self.ffn_dim, self.eps = dim, num_heads, ffn_dim, eps
        self.self_attn = AttentionParams(dim, num_heads, device, fused=("q", "k", "v"))
        self.cross_attn = AttentionParams(dim, num_heads, device, fused=("k", "v"), image=has_image_input)
        self.norm3 = LayerNormAffine(dim, device)
        self.ffn = Sequential3(Linear(dim, ffn_dim, device=device), Linear(ffn_dim, dim, device=device))
        self.modulation = _param(1, 6, dim, device=device)

    def forward(self, x, t_mod, rc, hint=None, hint_scale=1.0, only_batch=None, shared_prefix=False):
        """x: [B*S, D] updated in place.  t_mod: [B, 6, D] ([2 B, 6, D] with rc.seg_rows: sample b's two
        segments' rows at 2 b and 2 b + 1).  hint: [B*S, D] added after the block.
        only_batch: run the block for that CFG sample only (skip-layer guidance leaves the others'
        rows untouched).  Every GEMM fuses its epilogue (residual, gate, hint); each LayerNorm is a pass
        of its own.

        Four phases per micro-batch: (1) LN1 + q/k/v + QK-RMSNorm/RoPE, (2) self-attention,
        (3) o-proj (gated residual) + LN3, (4) cross-attention, FFN (gated residual + VACE hint).
        Without SP the whole CFG batch is one micro-batch.  Under Ulysses SP with overlap on, each
        CFG sample is its own micro-batch for phases 1-3, issued 1(0) 1(1) 2(0) 2(1) 3(0) 3(1): sample
        0's q|k|v all-to-all runs under sample 1's projections, sample 1's under sample 0's
        attention, sample 0's return exchange under sample 1's attention and sample 1's under sample
        0's o-proj; phase 4 then runs once on both samples' rows (GEMMs of 2S/p rows instead of two
        of S/p: host option sp_merge_ffn=0 keeps it per sample).

        shared_prefix (r6): the caller guarantees that every CFG sample's rows of x and of t_mod are
        equal (the first DiT block and the first VACE block, when the latents, the timestep and the VACE
        context are shared -- they differ only through the context, which phase 4 first reads), so
        phases 1-3 run on sample 0's rows alone and their outputs (x after the gated o-proj, the LN3
        rows) are copied to the other samples before phase 4 runs on all rows -- its cross-attention
        query too comes from sample 0's rows alone: the same per-row arithmetic, bit-identical
        (tests/test_model_gpu.py), half the self-attention of those blocks."""
        B, S, D, ws = rc.batch, rc.seq, self.dim, rc.ws
        # one buffer for every block: mod_add and every kernel that reads mod (the LayerNorms, the
        # gated GEMM epilogues) are enqueued on the current stream; side streams carry collectives only
        nm = 2 if rc.seg_rows else 1
        mod = ws.get("mod", (nm * B, 6, D))
        K.mod_add(self.modulation.view(6, D), t_mod, mod, 6 * D, D)   # :218-219
        sp = rc.sp
        shared = shared_prefix and B > 1 and only_batch is None and bool(host_option("cfg_prefix"))
        if only_batch is not None:
            parts = [self._part(x, mod, rc, only_batch, 1, hint, f".{only_batch}")]
        elif shared:
            parts = [self._part(x, mod, rc, 0, 1, hint, ".0")]
        elif sp is not None and B > 1 and getattr(sp, "overlap", False):
            parts = [self._part(x, mod, rc, b, 1, hint, f".{b}") for b in range(B)]
        else:
            parts = [self._part(x, mod, rc, 0, B, hint, "")]
        # phase 4 on all rows at once (the overlapped SP micro-batches, the shared prefix)
        tail = self._part(x, mod, rc, 0, B, hint, "") if shared or (len(parts) > 1 and
                                                                    host_option("sp_merge_ffn")) else None
        for p in parts:
            self._phase_qkv(p, rc)
        for p in parts:
            self._phase_attn(p, rc)
        for p in parts:
            self._phase_o(p, rc, direct=tail is None)
            if tail is None:
                self._phase_cross_ffn(p, rc, hint_scale)
        if shared:                          # sample 0's phase 1-3 results are every sample's: x, and the
            xs = x.view(B, S, D)            # cross-attention query (from sample 0's LN3 rows in h)
            xs[1:].copy_(xs[0:1].expand(B - 1, S, D))
            tail["shared_q"] = True
        if tail is not None:
            self._phase_cross_ffn(tail, rc, hint_scale)
        return x

    def _part(self, x, mod, rc, b0, nb, hint, tag):
        S, D, L, ws = rc.seq, self.dim, rc.ctx_len, rc.ws
        r0, M = b0 * S, nb * S
        nm = 2 if rc.seg_rows else 1
        p = dict(nb=nb, M=M, x=x[r0:r0 + M], mod=mod[nm * b0:nm * (b0 + nb)], ctx=rc.ctx[b0 * L:(b0 + nb) * L],
                 hint=None if hint is None else hint[r0:r0 + M], tag=tag)
        if rc.img is not None:          # this part's image rows: the shared set, or its samples' own
            p["img"] = rc.img if rc.img_batch == 1 else rc.img[b0 * IMG_TOKENS:(b0 + nb) * IMG_TOKENS]
        for n in ("h", "q", "k", "v", "o"):     # row slices of the all-samples buffers
            p[n] = ws.get(n, (rc.batch * S, D))[r0:r0 + M]
        return p

    def _phase_qkv(self, p, rc):
        # --- self-attention inputs (wan_video_dit.py:225-226, :140-145)
        S, D, eps, ws = rc.seq, self.dim, self.eps, rc.ws
        mod, h, q, k, v = p["mod"], p["h"], p["q"], p["k"], p["v"]
        sa = self.self_attn
        h = ln_into(p["x"], h, ws, sa, eps, shift=mod[:, 0], scale=mod[:, 1], mod_bstride=6 * D,
                    rows_per_batch=S, **rc.seg)
        qkv = fused_linear(sa, h, ws, "qkv" + p["tag"])
        if qkv is not None:            # one GEMM; q/k/v are column slices of [M, 3D]
            q, k, v = p["q"], p["k"], p["v"] = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        else:
            linear(sa.q, h, q, ws)
            linear(sa.k, h, k, ws)
            linear(sa.v, h, v, ws)
        K.rmsnorm_rope(q, sa.norm_q.weight, eps, rope=rc.rope, grid=rc.grid, rows_per_batch=S,
                       token_offset=rc.token_offset)
        K.rmsnorm_rope(k, sa.norm_k.weight, eps, rope=rc.rope, grid=rc.grid, rows_per_batch=S,
                       token_offset=rc.token_offset)
        if rc.sp is not None:
            p["xchg"] = rc.sp.exchange_start(q, k, v, self.num_heads, p["nb"], p["tag"])

    def _phase_attn(self, p, rc):
        if rc.sp is not None:
            rc.sp.attend(p["xchg"])
        else:
            ev = TIMER.start("self_attn", attn_flops(p["q"], p["k"], p["nb"]))
            K.attention(p["q"], p["k"], p["v"], p["o"], self.num_heads, p["nb"])
            TIMER.stop(ev)

    def _phase_o(self, p, rc, direct=True):
        """direct: this part's cross-attention runs next (its LN3 may go straight into an fp8 cross-q's
        quantised input); False: the merged SP tail reads the bf16 LN3 rows of every part."""
        S, D, eps, ws = rc.seq, self.dim, self.eps, rc.ws
        x, mod, h, o = p["x"], p["mod"], p["h"], p["o"]
        if rc.sp is not None:
            rc.sp.finish(p["xchg"], o)
        linear(self.self_attn.o, o, x, ws, epilogue=K.VS_EPI_GATE_RES, residual=x, gate=mod[:, 2],
               gate_bstride=6 * D, rows_per_batch=S, **rc.seg)
        # --- cross-attention (wan_video_dit.py:227, :171-186)
        p["h3"] = ln_into(x, h, ws, self.cross_attn.q if direct else None, eps, weight=self.norm3.weight,
                          bias=self.norm3.bias)

    def _phase_cross_ffn(self, p, rc, hint_scale):
        S, D, eps, ws = rc.seq, self.dim, self.eps, rc.ws
        x, mod, h, q, o, nb, M = p["x"], p["mod"], p["h"], p["q"], p["o"], p["nb"], p["M"]
        ca = self.cross_attn
        L = rc.ctx_len
        if p.get("shared_q"):               # equal rows per sample (shared prefix): one sample's query
            linear(ca.q, h[:S], q[:S], ws)
            K.rmsnorm_rope(q[:S], ca.norm_q.weight, eps)
            q.view(nb, S, D)[1:].copy_(q[:S].unsqueeze(0).expand(nb - 1, S, D))
        else:
            linear(ca.q, p.pop("h3", h), q, ws)
            K.rmsnorm_rope(q, ca.norm_q.weight, eps)
        kv = fused_linear(ca, p["ctx"], ws, "kvc" + p["tag"])
        if kv is not None:
            kc, vc = kv[:, :D], kv[:, D:]
        else:
            kc, vc = ws.get("kc" + p["tag"], (nb * L, D)), ws.get("vc" + p["tag"], (nb * L, D))
            linear(ca.k, p["ctx"], kc, ws)
            linear(ca.v, p["ctx"], vc, ws)
        K.rmsnorm_rope(kc, ca.norm_k.weight, eps)
        K.attention(q, kc, vc, o, self.num_heads, nb)
        if ca.has_image_input:
            self._image_attn(p, rc, q, o)
        linear(ca.o, o, x, ws, epilogue=K.VS_EPI_RES, residual=x)
        # --- FFN (wan_video_dit.py:228-229) + VACE hint (wan_video_new.py:1450)
        h = ln_into(x, h, ws, self.ffn[0], eps, shift=mod[:, 3], scale=mod[:, 4], mod_bstride=6 * D,
                    rows_per_batch=S, **rc.seg)
        f = ws.get("f" + p["tag"], (M, self.ffn_dim))
        linear(self.ffn[0], h, f, ws, epilogue=K.VS_EPI_GELU)
        linear(self.ffn[2], f, x, ws, epilogue=K.VS_EPI_GATE_RES, residual=x,
               gate=mod[:, 5], gate_bstride=6 * D, rows_per_batch=S, hint=p["hint"], hint_scale=hint_scale,
               **rc.seg)


    def _image_attn(self, p, rc, q, o):
        """o += attention(q, k_img, v_img) over the 257 embedded image tokens (wan_video_dit.py:181-185),
        after the text attention has written o.  k_img | v_img come from one GEMM over the image rows
        -- once for all CFG samples when they share the image (key batch stride 0).  Host option
        img_attn_fused 1: vs_attn_fwd_add adds in its O store; 0: attention into a scratch buffer and
        an axpy pass (kernels that predate the fused one; bit-identical with attn_nc=0, attn_impl=8)."""
        ws, D, eps, nb, ca = rc.ws, self.dim, self.eps, p["nb"], self.cross_attn
        img = p.get("img")
        if img is None:
            raise ValueError("a DiT with has_image_input needs clip_feature (the embedded image tokens)")
        shared = rc.img_batch == 1
        kv = fused_img_linear(ca, img, ws, "kvi" + p["tag"])
        if kv is not None:
            ki, vi = kv[:, :D], kv[:, D:]
        else:
            ki, vi = ws.get("ki" + p["tag"], (img.shape[0], D)), ws.get("vi" + p["tag"], (img.shape[0], D))
            linear(ca.k_img, img, ki, ws)
            linear(ca.v_img, img, vi, ws)
        K.rmsnorm_rope(ki, ca.norm_k_img.weight, eps)
        if host_option("img_attn_fused"):
            K.attention_add(q, ki, vi, o, self.num_heads, nb, shared_kv=shared)
        else:
            oi = ws.get("o_img", (rc.batch * rc.seq, D))[:p["M"]]
            K.attention(q, ki, vi, oi, self.num_heads, nb, shared_kv=shared)
            K.axpy(o, oi, 1.0)


class Head(nn.Module):
    """wan_video_dit.py:253-269."""

    def __init__(self, dim, out_dim, patch_size, eps, device=None):
        super().__init__()
        self.dim, self.out_dim, self.eps = dim, out_dim, eps
        self.head = Linear(dim, out_dim * math.prod(patch_size), device=device)
        self.modulation = _param(1, 2, dim, device=device)

    def forward(self, x, t, rc):
        B, S, D, ws = rc.batch, rc.seq, self.dim, rc.ws
        h = ws.get("h", (B * S, D))
        # :267, a t row per sample; with rc.seg_rows (:263-265) t is [2 B, D]: a row per (sample, segment)
        hm = ws.get("head_mod", ((2 if rc.seg_rows else 1) * B, 2, D))
        K.mod_add(self.modulation.view(2, D), t, hm, D, 0)
        ln_into(x, h, ws, None, self.eps, shift=hm[:, 0], scale=hm[:, 1], mod_bstride=2 * D, rows_per_batch=S,
                **rc.seg)
        out = ws.get("head_out", (B * S, self.head.out_features))
        K.gemm(h, self.head.weight, out, bias=self.head.bias)
        return out


def rope_table(head_dim=128, end=1024, theta=10000.0, device=None):
    """float32 [end, head_dim/2, 2] (cos, sin) of the 3-D RoPE (wan_video_dit.py:75-89), from fp64."""
    def freqs(dim):
        return 1.0 / (theta ** (torch.arange(0, dim, 2)[: dim // 2].double() / dim))
    f = torch.cat([freqs(head_dim - 2 * (head_dim // 3)), freqs(head_dim // 3), freqs(head_dim // 3)])
    ang = torch.outer(torch.arange(end).double(), f)
    tab = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).float()
    return tab.to(device)


class ImgEmbProj(nn.Module):
    """MLP.proj (wan_video_dit.py:235-241): LayerNorm, Linear, GELU, Linear, LayerNorm at indices 0, 1, 3, 4."""

    def __init__(self, in_dim, out_dim, device=None):
        super().__init__()
        self.add_module("0", LayerNormAffine(in_dim, device))
        self.add_module("1", Linear(in_dim, in_dim, device=device))
        self.add_module("3", Linear(in_dim, out_dim, device=device))
        self.add_module("4", LayerNormAffine(out_dim, device))

    def __getitem__(self, i):
        return getattr(self, str(i))


class ImgEmb(nn.Module):
    """MLP(1280, dim, has_pos_emb) parameters (wan_video_dit.py:232-249): the CLIP-feature embedding."""

    def __init__(self, in_dim, out_dim, has_pos_emb=False, device=None):
        super().__init__()
        self.in_dim, self.out_dim = in_dim, out_dim
        self.proj = ImgEmbProj(in_dim, out_dim, device)
        self.has_pos_emb = has_pos_emb
        if has_pos_emb:
            self.emb_pos = _param(1, 2 * IMG_TOKENS, in_dim, device=device)


class RefConv(nn.Module):
    """Conv2d(16, dim, k = s = 2) parameters (wan_video_dit.py:331): the reference image's latents -> tokens."""

    def __init__(self, dim, device=None):
        super().__init__()
        self.weight = _param(dim, 16, 2, 2, device=device)
        self.bias = _param(dim, device=device)


class Conv2dParams(nn.Module):
    def __init__(self, cin, cout, k, device=None):
        super().__init__()
        self.weight = _param(cout, cin, k, k, device=device)
        self.bias = _param(cout, device=device)


class AdapterResidualBlock(nn.Module):
    """ResidualBlock(dim) parameters (wan_video_camera_controller.py:63-75): two 3x3 convs, padding 1."""

    def __init__(self, dim, device=None):
        super().__init__()
        self.conv1 = Conv2dParams(dim, dim, 3, device)
        self.conv2 = Conv2dParams(dim, dim, 3, device)


class SimpleAdapter(nn.Module):
    """The camera control adapter (wan_video_camera_controller.py:8-44) under the reference's parameter
    names: PixelUnshuffle(8), conv = Conv2d(64 in_dim, dim, k = s = 2), one ResidualBlock.  forward runs on
    token rows: the [T h w, dim] buffer is the 3x3 convs' channels-last layout with n = T frames."""

    def __init__(self, in_dim, out_dim, device=None, num_residual_blocks=1):
        super().__init__()
        if num_residual_blocks != 1:
            raise NotImplementedError("SimpleAdapter: one residual block (every published layout)")
        self.in_dim, self.out_dim = in_dim, out_dim
        self.conv = Conv2dParams(in_dim * 64, out_dim, 2, device)
        self.residual_blocks = nn.ModuleList([AdapterResidualBlock(out_dim, device)])
        self._cw = {}

    def _conv_weight(self, name, conv):
        """The 3x3 weight re-laid out for vs_vae_conv (vae.ConvW), once per loaded weight."""
        from .vae import ConvW
        key = (conv.weight.data_ptr(), conv.weight._version, conv.bias.data_ptr(), conv.bias._version)
        have = self._cw.get(name)
        if have is None or have[0] != key:
            have = (key, ConvW(conv.weight, conv.bias, conv.weight.device))
            self._cw[name] = have
        return have[1]

    def forward(self, control_camera_latents_input):
        """[1, in_dim, T, H, W] (H, W pixels) -> [T (H/16)(W/16), dim] token rows, in the patch embedding's
        row order: SimpleAdapter.forward's x_conv, relu(conv1), conv2 + bias, += residual, each a bf16
        tensor as the reference's bf16 modules make them.  Once per call, outside the captured step: the
        buffers are the caller's (the im2col is 400 MB at 832x480x81), not the Workspace's."""
        from .vae import conv as vae_conv
        x = control_camera_latents_input
        if x.dim() != 5 or x.shape[0] != 1 or x.shape[1] != self.in_dim or x.shape[3] % 16 or x.shape[4] % 16:
            raise ValueError(f"control_camera_latents_input: expected [1, {self.in_dim}, T, H, W] with H, W multiples "
                             f"of 16, got {tuple(x.shape)}")
        _, C, T, H, W = x.shape
        h, w, D = H // 16, W // 16, self.out_dim
        M = T * h * w
        dev = self.conv.weight.device

        def buf(cols):
            return torch.empty((M, cols), device=dev, dtype=BF16)
        cols = buf(256 * C)
        K.camera_im2col(x.to(device=dev, dtype=BF16).contiguous()[0], cols)
        u = buf(D)
        K.gemm(cols, self.conv.weight.view(D, 256 * C), u, bias=self.conv.bias)
        blk = self.residual_blocks[0]
        a = buf(D)
        vae_conv(u.view(T, 1, h, w, D), self._conv_weight("conv1", blk.conv1), (1, h, w), pad=(0, 1, 1),
                 y=a.view(T, 1, h, w, D))
        K.relu(a)
        out = buf(D)
        vae_conv(a.view(T, 1, h, w, D), self._conv_weight("conv2", blk.conv2), (1, h, w), pad=(0, 1, 1),
                 y=out.view(T, 1, h, w, D), res=u.view(T, 1, h, w, D))
        return out


CLIP_DIM = 1280       # clip_feature_dim (wan_video_dit.py:322)
IMG_EMB_EPS = 1e-5    # nn.LayerNorm's default eps, which MLP.proj's two LayerNorms keep


class WanModel(nn.Module):
    """wan_video_dit.py:272-337: the T2V / VACE layout (in_dim 16) and the image-conditioned ones --
    in_dim > 16 (the VAE-embedded image `y` concatenated behind the latents: I2V, FLF2V, Fun-InP,
    Wan2.2-I2V-A14B; or the 48 latent channels of Wan2.2-TI2V-5B, which takes no `y`:
    fuse_vae_embedding_in_latents / seperated_timestep) with or without the CLIP image branch (has_image_input: img_emb + the blocks'
    k_img / v_img / norm_k_img; has_image_pos_emb: img_emb.emb_pos over 514 tokens).  The Wan-Fun control
    layouts (in_dim > 16, out_dim 16) add has_ref_conv (ref_conv: the reference image's latents -> tokens in
    front of the sequence) and add_control_adapter (control_adapter: the camera rays -> rows added to the patch
    embedding's), :330-345."""

    def __init__(self, dim, in_dim, ffn_dim, out_dim, text_dim, freq_dim, eps, patch_size, num_heads,
                 num_layers, has_image_input=False, has_image_pos_emb=False, has_ref_conv=False,
                 add_control_adapter=False, seperated_timestep=False, require_vae_embedding=True,
                 require_clip_embedding=True, fuse_vae_embedding_in_latents=False, in_dim_control_adapter=24,
                 device=None, **kwargs):
        super().__init__()
        for name, on in (("has_ref_conv", has_ref_conv), ("add_control_adapter", add_control_adapter)):
            # ref_conv reads 16-channel Wan2.1 latents and every Fun-Control layout keeps the control / image
            # channels in y: in_dim > 16 with 16 output channels (wan_video_dit.py:610-748)
            if on and not (in_dim > 16 and out_dim == 16):
                raise NotImplementedError(f"WanModel({name}=True) (Fun-Control reference conv, camera control) "
                                          f"with in_dim {in_dim} / out_dim {out_dim} is not in this build: the "
                                          f"Fun-Control layouts have in_dim > 16 and out_dim 16")
        if bool(seperated_timestep) != bool(fuse_vae_embedding_in_latents):
            # Wan2.2-TI2V-5B, the one layout with either flag, sets both; each alone is another model
            raise NotImplementedError("WanModel: seperated_timestep and fuse_vae_embedding_in_latents go together "
                                      "(Wan2.2-TI2V-5B); one without the other is not in this build")
        if dim // num_heads != 128:
            raise NotImplementedError("head_dim must be 128 (all Wan2.1 models)")
        if in_dim < 16:
            raise ValueError(f"in_dim {in_dim}: the 16 latent channels come first")
        if has_image_pos_emb and not has_image_input:
            raise ValueError("has_image_pos_emb needs has_image_input")
        self.dim, self.in_dim, self.ffn_dim, self.out_dim = dim, in_dim, ffn_dim, out_dim
        self.text_dim, self.freq_dim, self.eps, self.num_heads = text_dim, freq_dim, eps, num_heads
        self.patch_size = tuple(patch_size)
        self.has_image_input = bool(has_image_input)
        self.has_image_pos_emb = bool(has_image_pos_emb)
        # Wan2.2-TI2V-5B: the first latent frame holds the clean image latents and its tokens run at
        # timestep 0 (model_fn_wan_video(fuse_vae_embedding_in_latents=True))
        self.seperated_timestep = bool(seperated_timestep)
        self.require_vae_embedding = bool(require_vae_embedding)
        self.require_clip_embedding = bool(require_clip_embedding)
        self.fuse_vae_embedding_in_latents = bool(fuse_vae_embedding_in_latents)
        self.patch_embedding = PatchEmbed(in_dim, dim, device)
        self.text_embedding = Sequential3(Linear(text_dim, dim, device=device), Linear(dim, dim, device=device))
        self.time_embedding = Sequential3(Linear(freq_dim, dim, device=device), Linear(dim, dim, device=device))
        self.time_projection = nn.Module()
        self.time_projection.add_module("1", Linear(dim, 6 * dim, device=device))
        self.blocks = nn.ModuleList([DiTBlock(dim, num_heads, ffn_dim, eps, device, has_image_input=has_image_input)
                                     for _ in range(num_layers)])
        self.head = Head(dim, out_dim, patch_size, eps, device)
        if has_image_input:
            self.img_emb = ImgEmb(CLIP_DIM, dim, has_pos_emb=has_image_pos_emb, device=device)
        # Wan-Fun control (wan_video_dit.py:330-337): the reference image's tokens, the camera adapter
        self.has_ref_conv = bool(has_ref_conv)
        if has_ref_conv:
            self.ref_conv = RefConv(dim, device)
        self.control_adapter = SimpleAdapter(in_dim_control_adapter, dim, device) if add_control_adapter else None
        self._rope = None

    def ref_tokens(self, reference_latents, ws):
        """reference_latents [Br, 16, h, w] -> [Br * (h/2)(w/2), D]: ref_conv(...).flatten(2).transpose(1, 2)
        (wan_video_new.py:1388) as the im2col of one frame and one GEMM with bias, the conv's rounding."""
        Br, C, H, W = reference_latents.shape
        n = (H // 2) * (W // 2)
        cols = ws.get("ref.cols", (Br * n, 4 * C))
        K.patchify(reference_latents.to(device=self.ref_conv.weight.device, dtype=BF16).contiguous().view(Br, C, 1, H, W),
                   cols)
        out = ws.get("ref.out", (Br * n, self.dim))
        return K.gemm(cols, self.ref_conv.weight.view(self.dim, 4 * C), out, bias=self.ref_conv.bias)

    def img_embed(self, clip_feature, ws):
        """clip_feature [Bc, N, 1280] -> [Bc*N, D]: MLP.forward (wan_video_dit.py:246-249) as
        [+ emb_pos], LayerNorm-affine over 1280, Linear, erf-GELU, Linear, LayerNorm-affine over D; every
        step rounds to bf16 as the reference's bf16 modules do."""
        e = self.img_emb
        Bc, N, C = clip_feature.shape
        if C != CLIP_DIM or N not in (IMG_TOKENS, 2 * IMG_TOKENS):
            raise ValueError(f"clip_feature: expected [B, {IMG_TOKENS} or {2 * IMG_TOKENS}, {CLIP_DIM}], got "
                             f"{tuple(clip_feature.shape)}")
        x = clip_feature.to(BF16).contiguous()
        if e.has_pos_emb:
            if N != 2 * IMG_TOKENS:     # x + emb_pos (1, 514, 1280) broadcasts over the batch only (:247-248)
                raise ValueError(f"img_emb.emb_pos covers {2 * IMG_TOKENS} tokens, clip_feature has {N}")
            x = K.mod_add(e.emb_pos.view(N, C), x, ws.get("img_x", (Bc, N, C)), N * C, C)
        M = Bc * N
        h = ws.get("img_h", (M, C))
        K.layernorm_modulate(x.view(M, C), h, IMG_EMB_EPS, weight=e.proj[0].weight, bias=e.proj[0].bias)
        u = ws.get("img_u", (M, C))
        K.gemm(h, e.proj[1].weight, u, bias=e.proj[1].bias)
        K.gelu_erf(u)
        v = ws.get("img_v", (M, self.dim))
        K.gemm(u, e.proj[3].weight, v, bias=e.proj[3].bias)
        out = ws.get("img_emb", (M, self.dim))
        K.layernorm_modulate(v, out, IMG_EMB_EPS, weight=e.proj[4].weight, bias=e.proj[4].bias)
        return out

    def rope(self, device):
        if self._rope is None or self._rope.device != torch.device(device):
            self._rope = rope_table(self.dim // self.num_heads, device=device)
        return self._rope

    def time_embed(self, timestep, ws):
        """t [B,D], t_mod [B,6,D] (wan_video_new.py:1351-1352)."""
        B, D = timestep.shape[0], self.dim
        s = ws.get("sinus", (B, self.freq_dim))
        K.time_sinusoid(timestep.contiguous(), s)
        u = ws.get("t_u", (B, D))
        K.gemm(s, self.time_embedding[0].weight, u, epilogue=K.VS_EPI_SILU, bias=self.time_embedding[0].bias)
        t = ws.get("t", (B, D))
        K.gemm(u, self.time_embedding[2].weight, t, bias=self.time_embedding[2].bias)
        st = ws.get("t_silu", (B, D))
        K.gemm(u, self.time_embedding[2].weight, st, epilogue=K.VS_EPI_SILU, bias=self.time_embedding[2].bias)
        tm = ws.get("t_mod", (B, 6 * D))
        proj = getattr(self.time_projection, "1")
        K.gemm(st, proj.weight, tm, bias=proj.bias)
        return t, tm.view(B, 6, D)

    def text_embed(self, context, ws):
        """[B*L, text_dim] -> [B*L, D] (wan_video_dit.py:308-312)."""
        BL = context.shape[0] * context.shape[1]
        c = context.reshape(BL, self.text_dim).contiguous()
        h = ws.get("ctx_h", (BL, self.dim))
        K.gemm(c, self.text_embedding[0].weight, h, epilogue=K.VS_EPI_GELU, bias=self.text_embedding[0].bias)
        out = ws.get("ctx", (BL, self.dim))
        K.gemm(h, self.text_embedding[2].weight, out, bias=self.text_embedding[2].bias)
        return out


class VaceWanAttentionBlock(DiTBlock):
    """wan_video_vace.py:5-24."""

    def __init__(self, dim, num_heads, ffn_dim, eps=1e-6, block_id=0, device=None):
        super().__init__(dim, num_heads, ffn_dim, eps, device)
        self.block_id = block_id
        if block_id == 0:
            self.before_proj = Linear(dim, dim, device=device)
        self.after_proj = Linear(dim, dim, device=device)


class VaceWanModel(nn.Module):
    """wan_video_vace.py:27-87; the hints are computed on the (possibly SP-sharded) token rows."""

    def __init__(self, vace_layers=tuple(range(0, 30, 2)), vace_in_dim=96, patch_size=(1, 2, 2),
                 has_image_input=False, dim=1536, num_heads=12, ffn_dim=8960, eps=1e-6, device=None):
        super().__init__()
        self.vace_layers = tuple(vace_layers)
        self.vace_in_dim = vace_in_dim
        self.vace_layers_mapping = {i: n for n, i in enumerate(self.vace_layers)}
        self.vace_blocks = nn.ModuleList([
            VaceWanAttentionBlock(dim, num_heads, ffn_dim, eps, block_id=i, device=device) for i in self.vace_layers])
        self.vace_patch_embedding = PatchEmbed(vace_in_dim, dim, device)
        self.dim = dim

    def forward(self, x, vace_cols_out, t_mod, rc, shared_prefix=False):
        """x: patch-embedded main tokens [B*S, D]; vace_cols_out: patch-embedded control tokens
        [B*S, D] (overwritten, becomes c).  Returns the list of hint buffers [B*S, D].  shared_prefix:
        every CFG sample's rows of x, of the control tokens and of t_mod are equal (DiTBlock)."""
        ws, D = rc.ws, self.dim
        M = rc.batch * rc.seq
        c = vace_cols_out
        hints = []
        # with a shared prefix block 0 reads sample 0's rows of c0 alone and overwrites the others
        # after its self-attention half, so before_proj runs on those rows only
        rows = rc.seq if shared_prefix and rc.batch > 1 and host_option("cfg_prefix") else M
        for n, blk in enumerate(self.vace_blocks):
            if n == 0:
                c0 = ws.get("vace_c", (M, D))
                linear(blk.before_proj, c[:rows], c0[:rows], ws, epilogue=K.VS_EPI_RES, residual=x[:rows])
                c = c0
            blk(c, t_mod, rc, shared_prefix=shared_prefix and n == 0)
            hint = ws.get(f"vace_hint{n}", (M, D))
            linear(blk.after_proj, c, hint, ws)
            hints.append(hint)
        return hints


class CausalConv1dParams(nn.Module):
    """wan_video_animate_adapter.py:50-63: Conv1d(cin, cout, 3) behind two replicate-padded frames, under
    the reference's name `conv`.  Run as a GEMM over gathered rows: gemm_weight() is the weight as
    (cout, Kp), column k cin + c = weight[:, c, k], Kp = 3 cin rounded up to the GEMM's K step of 64."""

    def __init__(self, cin, cout, stride, device=None):
        super().__init__()
        self.cin, self.cout, self.stride = cin, cout, stride
        self.conv = nn.Module()
        self.conv.weight = _param(cout, cin, 3, device=device)
        self.conv.bias = _param(cout, device=device)
        self._w = self._w_of = None

    def gemm_weight(self):
        key = (self.conv.weight.data_ptr(), self.conv.weight._version)
        if self._w is None or self._w_of != key:
            k = 3 * self.cin
            w = torch.zeros((self.cout, (k + 63) // 64 * 64), device=self.conv.weight.device, dtype=BF16)
            w[:, :k].copy_(self.conv.weight.detach().permute(0, 2, 1).reshape(self.cout, k))
            self._w, self._w_of = w, key
        return self._w

    def forward(self, x, tag, ws):
        """x [G, T, cin] -> [G, T', cout], T' = (T - 1) // stride + 1: output frame t reads the frames
        max(t stride + k - 2, 0), k = 0..2 (the row gather is indexing; the arithmetic is vs_gemm's)."""
        G, T, C = x.shape
        To = (T - 1) // self.stride + 1
        w = self.gemm_weight()
        src = (torch.arange(To, device=x.device).view(To, 1) * self.stride +
               torch.arange(3, device=x.device).view(1, 3) - 2).clamp_(min=0)
        cols = ws.get(tag + ".cols", (G * To, w.shape[1]))
        if w.shape[1] != 3 * C:
            cols.zero_()
        cols.view(G, To, -1)[:, :, :3 * C].copy_(x[:, src].reshape(G, To, 3 * C))
        out = ws.get(tag + ".out", (G * To, self.cout))
        K.gemm(cols, w, out, bias=self.conv.bias)
        return out.view(G, To, self.cout)


class FaceEncoder(nn.Module):
    """wan_video_animate_adapter.py:67-114: motion vectors [B, T, in_dim] -> [B, T', num_heads + 1,
    hidden_dim] motion tokens (T' = T through strides 1, 2, 2), the last token of every frame the learned
    padding token.  The three LayerNorms carry no parameters."""
    WIDTH = 1024

    def __init__(self, in_dim, hidden_dim, num_heads=4, device=None):
        super().__init__()
        self.in_dim, self.hidden_dim, self.num_heads = in_dim, hidden_dim, num_heads
        self.conv1_local = CausalConv1dParams(in_dim, self.WIDTH * num_heads, 1, device)
        self.conv2 = CausalConv1dParams(self.WIDTH, self.WIDTH, 2, device)
        self.conv3 = CausalConv1dParams(self.WIDTH, self.WIDTH, 2, device)
        self.out_proj = Linear(self.WIDTH, hidden_dim, device=device)
        self.padding_tokens = _param(1, 1, 1, hidden_dim, device=device)

    def forward(self, motion, ws):
        B, T, C = motion.shape
        if C != self.in_dim:
            raise ValueError(f"face motion: expected [B, T, {self.in_dim}], got {tuple(motion.shape)}")
        n, Wd = self.num_heads, self.WIDTH
        x = self.conv1_local(motion.to(BF16), "face.c1", ws)                    # [B, T, n Wd]
        # "b (n c) t -> (b n) t c": each head's 1024 channels become a sequence of their own
        h = ws.get("face.h1", (B * n, T, Wd))
        h.view(B, n, T, Wd).copy_(x.view(B, T, n, Wd).permute(0, 2, 1, 3))
        K.ln_silu(h.view(-1, Wd))
        x = self.conv2(h, "face.c2", ws)
        K.ln_silu(x.view(-1, Wd))
        x = self.conv3(x, "face.c3", ws)
        K.ln_silu(x.view(-1, Wd))
        To = x.shape[1]
        y = ws.get("face.proj", (B * n * To, self.hidden_dim))
        K.gemm(x.view(-1, Wd), self.out_proj.weight, y, bias=self.out_proj.bias)
        out = torch.empty((B, To, n + 1, self.hidden_dim), device=motion.device, dtype=BF16)
        out[:, :, :n].copy_(y.view(B, n, To, self.hidden_dim).permute(0, 2, 1, 3))
        out[:, :, n] = self.padding_tokens.view(self.hidden_dim)
        return out


class FaceBlock(nn.Module):
    """wan_video_animate_adapter.py:235-310 parameters (the two pre-norms carry none)."""

    def __init__(self, dim, num_heads, device=None):
        super().__init__()
        self.dim, self.num_heads = dim, num_heads
        self.linear1_kv = Linear(dim, 2 * dim, device=device)
        self.linear1_q = Linear(dim, dim, device=device)
        self.linear2 = Linear(dim, dim, device=device)
        self.q_norm = RMSNormW(dim // num_heads, device)
        self.k_norm = RMSNormW(dim // num_heads, device)


class FaceAdapter(nn.Module):
    def __init__(self, dim, num_heads, num_adapter_layers, device=None):
        super().__init__()
        self.fuser_blocks = nn.ModuleList([FaceBlock(dim, num_heads, device) for _ in range(num_adapter_layers)])


ANIMATE_EVERY = 5       # a fuser block after every fifth DiT block (wan_video_animate_adapter.py:646)
ANIMATE_PREFIXES = ("pose_patch_embedding.", "face_adapter.", "face_encoder.", "motion_encoder.")


class WanAnimateAdapter(nn.Module):
    """wan_video_animate_adapter.py:615-650 for any (dim, num_heads, num_layers): the pose latents' patch
    embedding, the face encoder and ceil(num_layers / 5) fuser blocks, under the reference's parameter
    names.  The motion encoder's tensors (face frames -> one 512-vector per frame) are kept unconverted in
    `motion_encoder`; encode_motion() builds vstyler.motion.MotionEncoder from them on first use, and the
    pipeline takes either the face frames (animate_face_video=) or the motion vectors themselves
    (animate_face_motion=).

    Once per call: pose_rows() (the residual rows of every step's patch-embedding GEMM), motion_tokens()
    and face_kv() (every fuser block's keys and values, K already through k_norm).  Per step, after block i
    with i % 5 == 0: after_block()."""

    def __init__(self, dim=5120, num_heads=40, num_layers=40, in_dim=512, eps=1e-6, device=None):
        super().__init__()
        if dim // num_heads != 128 or dim % num_heads:
            raise NotImplementedError("WanAnimateAdapter: head_dim must be 128")
        self.dim, self.num_heads, self.num_layers, self.eps = dim, num_heads, num_layers, eps
        self.pose_patch_embedding = PatchEmbed(16, dim, device)
        self.face_adapter = FaceAdapter(dim, num_heads, -(-num_layers // ANIMATE_EVERY), device)
        self.face_encoder = FaceEncoder(in_dim, dim, 4, device)
        self.motion_encoder = {}

    def load_state_dict(self, state_dict, strict=True, **kw):
        sd = dict(state_dict)
        self.motion_encoder = {k: sd.pop(k) for k in list(sd) if k.startswith("motion_encoder.")}
        return super().load_state_dict(sd, strict=strict, **kw)

    @property
    def motion_encoder(self):
        """The raw `motion_encoder.*` tensors, unconverted.  Assigning another dict drops the encoder built from
        the previous one (`motion_net`)."""
        return self.__dict__["_motion_encoder"]

    @motion_encoder.setter
    def motion_encoder(self, tensors):
        self.__dict__["_motion_encoder"] = tensors
        self.__dict__.pop("motion_net", None)

    def motion_size(self):
        """The face frame size of the motion encoder whose complete key set `motion_encoder` holds, or None."""
        from .motion import size_of
        return size_of(self.motion_encoder)

    def encode_motion(self, frames, chunk=None):
        """Face frames (uint8 [T, size, size, 3] or bf16 [3, T, size, size]) -> motion vectors [T, 512] bf16
        (vstyler.motion.MotionEncoder, the reference's motion_encoder.get_motion).  The encoder is built from
        the raw `motion_encoder` tensors on first use and kept as the plain attribute `motion_net` (no
        registered submodule: state_dict() stays without its keys).  NotImplementedError when those tensors
        are absent or incomplete."""
        from .motion import ENCODE_BS, MotionEncoder
        net = self.__dict__.get("motion_net")
        if net is None or net.source_keys != len(self.motion_encoder):        # (a dict edited in place, too)
            net = MotionEncoder(self.motion_encoder, device=self.face_encoder.out_proj.weight.device)
            net.source_keys = len(self.motion_encoder)
            self.__dict__["motion_net"] = net
        return net.encode(frames, ENCODE_BS if chunk is None else chunk)

    def pose_rows(self, pose_latents, frames, ws):
        """pose_latents [Bp, 16, frames - 1, H, W] -> [Bp * frames (H/2)(W/2), dim]: the pose patch
        embedding's rows at latent frames 1.. of every sample, zeros at frame 0
        (after_patch_embedding: x[:, :, 1:] += pose_patch_embedding(pose_latents)).  A tensor of its own."""
        p = self.pose_patch_embedding
        if pose_latents.dim() != 5 or pose_latents.shape[1] != 16 or pose_latents.shape[2] != frames - 1 or frames < 2:
            raise ValueError(f"pose_latents {tuple(pose_latents.shape)}: expected [B, 16, {frames} - 1, H, W] "
                             "(one latent frame fewer than the latents: frame 0 is the reference image's)")
        Bp, C, T, H, W = pose_latents.shape
        hw = (H // 2) * (W // 2)
        tok, _ = p(pose_latents.to(device=p.weight.device, dtype=BF16), ws, "pose")
        rows = torch.zeros((Bp, frames * hw, self.dim), device=tok.device, dtype=BF16)
        rows[:, hw:].copy_(tok.view(Bp, T * hw, self.dim))
        return rows.view(Bp * frames * hw, self.dim)

    def motion_tokens(self, motion, ws):
        """motion [B, T_face, in_dim] -> [B, T' + 1, N, dim]: the face encoder's tokens behind a zero frame
        (after_patch_embedding's pad_face)."""
        tok = self.face_encoder(motion.to(self.face_encoder.out_proj.weight.device), ws)
        B, To, N, D = tok.shape
        out = torch.zeros((B, To + 1, N, D), device=tok.device, dtype=BF16)
        out[:, 1:].copy_(tok)
        return out

    def face_kv(self, motion_vec, ws):
        """motion_vec [B, F, N, dim] -> one [B, F N, 2 dim] buffer per fuser block, columns [0, dim) the
        keys after k_norm and [dim, 2 dim) the values: pre_norm_motion (LayerNorm without affine: the zero
        frame stays zero), linear1_kv, the per-head RMSNorm of the K half.  The buffers belong to the
        workspace: a captured step reads them and the next call of the same shape overwrites them."""
        B, F, N, D = motion_vec.shape
        rows = motion_vec.reshape(B * F * N, D).contiguous()
        h = ws.get("animate.kv_h", (B * F * N, D))
        K.layernorm_modulate(rows, h, self.eps)
        out = []
        for i, fb in enumerate(self.face_adapter.fuser_blocks):
            kv = ws.get(f"animate.kv{i}", (B, F * N, 2 * D))
            K.gemm(h, fb.linear1_kv.weight, kv.view(B * F * N, 2 * D), bias=fb.linear1_kv.bias)
            K.head_rmsnorm(kv.view(B * F * N, 2 * D)[:, :D], fb.k_norm.weight, self.num_heads, self.eps)
            out.append(kv)
        return out

    def after_block(self, i, x, kv, rc):
        """after_transformer_block (:645-650) on the rows of x [B * S, dim] in place: LayerNorm without
        affine, linear1_q, vs_face_attn against this fuser block's keys / values, linear2 with the residual
        add fused.  Row-local: under Ulysses every rank runs it on its own rows (rc.token_offset)."""
        if i % ANIMATE_EVERY:
            return x
        fb = self.face_adapter.fuser_blocks[i // ANIMATE_EVERY]
        B, S, D, ws = rc.batch, rc.seq, self.dim, rc.ws
        k = kv[i // ANIMATE_EVERY]
        F, hw = rc.grid[0], rc.grid[1] * rc.grid[2]
        h = ln_into(x, ws.get("h", (B * S, D)), ws, fb.linear1_q, self.eps)
        q = ws.get("q", (B * S, D))
        linear(fb.linear1_q, h, q, ws)
        K.face_attn(q, k[:, :, :D], k[:, :, D:], fb.q_norm.weight, batch=B, num_heads=self.num_heads, frames=F,
                    tokens_per_frame=hw, nkeys=k.shape[1] // F, token_offset=rc.token_offset, eps=self.eps)
        linear(fb.linear2, q, x, ws, epilogue=K.VS_EPI_RES, residual=x)
        return x


def init_random_(module, seed=5, std=0.02):
    """Synthetic on-device init of SURVEY.md §8(d) (used by bench.py / smoke; real checkpoints load
    by name): N(0,std) weights, 0.01*N biases, modulation randn/sqrt(D), norm weights 1+0.1*N."""
    g = torch.Generator(device=next(module.parameters()).device).manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("modulation"):
                p.copy_(torch.randn(p.shape, generator=g, device=p.device) / p.shape[-1] ** 0.5)
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g, device=p.device))
            elif name.endswith("bias"):
                p.copy_(0.01 * torch.randn(p.shape, generator=g, device=p.device))
            else:
                p.normal_(0.0, std, generator=g)
    return module
