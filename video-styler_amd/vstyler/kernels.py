"""Typed wrappers over the C ABI: torch tensors in, launches on the current HIP stream.

PyTorch is used only for device memory and streams; every computation below is a kernel of
libvstyler.so.  Wrappers validate dtype/device/layout and raise ValueError before launching.
"""
import os
import ctypes

import torch

from . import _lib
from ._lib import VS_EPI_BIAS, VS_EPI_GELU, VS_EPI_SILU, VS_EPI_GATE_RES, VS_EPI_RES, VsEpilogue

BF16 = torch.bfloat16


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def set_option(name, value):
    """Select a path of libvstyler (include/vstyler.h VS_OPT_*, e.g. set_option("queue", 0));
    returns the previous value.  The defaults are the product configuration; tests and A/B probes
    use the others."""
    prev = _lib.load().vs_set_option(_lib.OPTIONS[name], int(value))
    if prev < 0:
        raise ValueError(f"vs_set_option: bad option {name}={value}")
    return prev


def get_option(name):
    return _lib.load().vs_get_option(_lib.OPTIONS[name])


class options:
    """Context manager: options(gemm_kernel=8, gemm_split=0) for the duration of a with-block."""

    def __init__(self, **kw):
        self.kw, self.saved = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.saved[k] = set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            set_option(k, v)
        return False


def apply_env_options():
    """VSTYLER_OPTS="queue=0,sp_comm=native": the one environment hook, read by the Python host
    (never by the library) so that A/B scripts can select paths of a whole run: host option names
    (vstyler.options) set the host's table, every other name a library option."""
    from .options import apply_spec
    apply_spec(os.environ.get("VSTYLER_OPTS", ""), set_option)


_SPLIT_WS = {}


def _split_ws(kind, t, nbytes=None):
    """Bind library scratch of `kind` (0 attention split tail, 1 GEMM split tail, 4 attention item
    flags, 5 GEMM tile and attention item queues; 2 and 3 are retired numbers no caller binds) for the
    current stream of t's device from the torch allocator (vs_split_workspace_bind: the library never
    allocates).  Re-bound larger when a bigger one is needed; never inside a graph capture (the
    library then takes its fallback)."""
    stream = _stream(t)
    key = (kind, t.device.index, stream)
    have = _SPLIT_WS.get(key)
    if nbytes is None:
        if have is not None:
            return
        nbytes = _lib.load().vs_split_workspace_bytes(kind)
        if nbytes <= 0:             # a kind the library does not use
            return
    elif have is not None and have.numel() >= nbytes:
        return
    if torch.cuda.is_current_stream_capturing():
        return
    # kinds 4 (attention item flags) and 5 (GEMM tile queues) must be zero when bound; the library
    # keeps them zero
    buf = (torch.zeros if kind in (4, 5) else torch.empty)(nbytes, dtype=torch.uint8, device=t.device)
    _lib.check(_lib.load().vs_split_workspace_bind(kind, buf.data_ptr(), nbytes, stream))
    _SPLIT_WS[key] = buf


def _req(t, name):
    if t.dtype != BF16:
        raise ValueError(f"{name}: expected bfloat16, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a device (cuda/hip) tensor")
    return t


def _rows(t, name):
    """(rows, cols, row_stride) of a 2-D view whose last dim is contiguous."""
    _req(t, name)
    if t.dim() < 2:
        raise ValueError(f"{name}: expected >=2-D tensor")
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: last dim must be contiguous")
    if t.dim() > 2:
        # all leading dims must collapse into one row index
        rows = 1
        for i in range(t.dim() - 1):
            rows *= t.shape[i]
        for i in range(t.dim() - 2):
            if t.stride(i) != t.stride(i + 1) * t.shape[i + 1]:
                raise ValueError(f"{name}: leading dims not collapsible")
        return rows, t.shape[-1], t.stride(-2)
    return t.shape[0], t.shape[1], t.stride(0)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _epilogue(bias, residual, gate, gate_bstride, hint, hint_scale, alpha, rows_per_batch, seg_rows=0):
    ep = VsEpilogue()
    ep.seg_rows = int(seg_rows)
    ep.bias = _ptr(bias)
    ep.hint_scale = float(hint_scale)
    ep.alpha = float(alpha)
    ep.rows_per_batch = int(rows_per_batch)
    if residual is not None:
        _, _, ldr = _rows(residual, "residual")
        ep.residual, ep.ld_res = residual.data_ptr(), ldr
    if gate is not None:
        ep.gate, ep.gate_bstride = gate.data_ptr(), int(gate_bstride)
    if hint is not None:
        _, _, ldh = _rows(hint, "hint")
        ep.hint, ep.ld_hint = hint.data_ptr(), ldh
    return ep


def gemm(a, w, out, epilogue=VS_EPI_BIAS, bias=None, residual=None, gate=None, gate_bstride=0,
         hint=None, hint_scale=1.0, alpha=1.0, rows_per_batch=0, a2=None, w2=None, seg_rows=0):
    """out[M,N] = epilogue(a[M,K] @ w[N,K]^T (+ a2 @ w2^T)) (see include/vstyler.h vs_gemm).
    seg_rows > 0 (VS_EPI_GATE_RES): gate holds two rows per sample, rows past the first seg_rows of a
    sample read the second (vs_epilogue.seg_rows)."""
    M, K, lda = _rows(a, "a")
    N, Kw, ldw = _rows(w, "w")
    Mo, No, ldc = _rows(out, "out")
    if Kw != K or Mo != M or No != N:
        raise ValueError(f"gemm shape mismatch a={tuple(a.shape)} w={tuple(w.shape)} out={tuple(out.shape)}")
    ep = _epilogue(bias, residual, gate, gate_bstride, hint, hint_scale, alpha, rows_per_batch, seg_rows)
    k2, lda2, ldw2 = 0, 0, 0
    if a2 is not None:
        _, k2, lda2 = _rows(a2, "a2")
        _, _, ldw2 = _rows(w2, "w2")
    if k2 == 0:
        _split_ws(1, a)
        _split_ws(5, a)
    _lib.check(_lib.load().vs_gemm(a.data_ptr(), lda, w.data_ptr(), ldw, out.data_ptr(), ldc, M, N, K,
                                   int(epilogue), ep, _ptr(a2), lda2, _ptr(w2), ldw2, k2, _stream(a)))
    return out


def _rows_u8(t, name):
    if t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 2 or t.stride(-1) != 1:
        raise ValueError(f"{name}: expected a 2-D row-major uint8 (e4m3 bits) device tensor")
    return t.shape[0], t.shape[1], t.stride(0)


def quant_fp8_rows(x, x8, scale):
    """x8 (uint8 e4m3 bits) and per-row fp32 scale of x, as fp8_linear (layers.py:124-137)."""
    M, K, ldx = _rows(x, "x")
    M8, K8, ld8 = _rows_u8(x8, "x8")
    if (M8, K8) != (M, K) or scale.dtype != torch.float32 or scale.numel() < M:
        raise ValueError("quant_fp8_rows: shape mismatch")
    _lib.check(_lib.load().vs_quant_fp8_rows(x.data_ptr(), ldx, x8.data_ptr(), ld8, scale.data_ptr(), M, K,
                                             _stream(x)))
    return x8, scale


def _lora_operands(a2, w2, m, n):
    """Shape / dtype checks of an un-merged LoRA phase's operands (a2 [m, k2], w2 [n, k2], bf16),
    on the tensors' metadata alone and before anything else of the call."""
    if a2 is None or w2 is None:
        raise ValueError("gemm_fp8: a2 and w2 go together")
    for t, name in ((a2, "a2"), (w2, "w2")):
        if t.dtype != BF16:
            raise ValueError(f"{name}: expected bfloat16, got {t.dtype}")
        if t.dim() != 2:
            raise ValueError(f"{name}: expected a 2-D tensor")
    if a2.shape[0] != m or w2.shape[0] != n or a2.shape[1] != w2.shape[1] or a2.shape[1] % 64:
        raise ValueError(f"gemm_fp8 LoRA shape mismatch a2={tuple(a2.shape)} w2={tuple(w2.shape)} for out [{m}, {n}] "
                         f"(rank a multiple of 64)")


def _weight_scale(scale_w, w8):
    """Checks of gemm_fp8's scale_w (fp32 [N], contiguous, on w8's device) on the tensors' metadata
    alone and before anything else of the call."""
    if not isinstance(scale_w, torch.Tensor) or scale_w.dtype != torch.float32:
        raise ValueError(f"scale_w: expected a float32 tensor, got {getattr(scale_w, 'dtype', type(scale_w))}")
    if scale_w.dim() != 1 or scale_w.shape[0] != w8.shape[0] or scale_w.stride(0) != 1:
        raise ValueError(f"scale_w: expected a contiguous [{w8.shape[0]}] vector (one scale per row of w8), got "
                         f"shape {tuple(scale_w.shape)} stride {tuple(scale_w.stride())}")
    if scale_w.device != w8.device:
        raise ValueError(f"scale_w: on {scale_w.device}, w8 on {w8.device}")


def gemm_fp8(a8, scale_a, w8, out, epilogue=VS_EPI_BIAS, bias=None, residual=None, gate=None, gate_bstride=0,
             hint=None, hint_scale=1.0, alpha=1.0, rows_per_batch=0, a2=None, w2=None, scale_w=None, seg_rows=0):
    """out = epilogue(scale_a[m] * (a8 @ w8^T) (+ a2 @ w2^T)) with e4m3 operands a8 / w8 and the bf16
    un-merged LoRA phase a2 [M, k2] / w2 [N, k2] (see vs_gemm_fp8, vs_gemm_fp8_lora).  scale_w (fp32
    [N]): the per-output-channel weight scale, out = epilogue(((a8 @ w8^T) * scale_w[n]) * scale_a[m]
    (+ a2 @ w2^T)) through vs_gemm_fp8_ws; None runs the entry points above.  seg_rows: as gemm()."""
    if scale_w is not None:
        _weight_scale(scale_w, w8)
    if a2 is not None or w2 is not None:
        _lora_operands(a2, w2, a8.shape[0], w8.shape[0])
    M, K, lda = _rows_u8(a8, "a8")
    N, Kw, ldw = _rows_u8(w8, "w8")
    Mo, No, ldc = _rows(out, "out")
    if Kw != K or Mo != M or No != N or scale_a.dtype != torch.float32:
        raise ValueError(f"gemm_fp8 shape mismatch a8={tuple(a8.shape)} w8={tuple(w8.shape)} out={tuple(out.shape)}")
    ep = _epilogue(bias, residual, gate, gate_bstride, hint, hint_scale, alpha, rows_per_batch, seg_rows)
    k2 = a2.shape[1] if a2 is not None else 0
    lda2 = ldw2 = 0
    if k2 > 0:                                      # whole-tile grid, no workspace
        _, _, lda2 = _rows(a2, "a2")
        _, _, ldw2 = _rows(w2, "w2")
    else:
        _split_ws(1, a8)                            # split tail of the MFMA kernel
        _split_ws(5, a8)                            # its tile queues
    lib = _lib.load()
    head = (a8.data_ptr(), lda, scale_a.data_ptr(), w8.data_ptr(), ldw)
    body = (out.data_ptr(), ldc, M, N, K, int(epilogue), ep)
    lora = (a2.data_ptr() if k2 else None, lda2, w2.data_ptr() if k2 else None, ldw2, k2)
    if scale_w is not None:
        _lib.check(lib.vs_gemm_fp8_ws(*head, scale_w.data_ptr(), *body, *lora, _stream(a8)))
    elif a2 is not None:                            # (an empty LoRA phase too: vs_gemm_fp8 by this entry)
        _lib.check(lib.vs_gemm_fp8_lora(*head, *body, *lora, _stream(a8)))
    else:
        _lib.check(lib.vs_gemm_fp8(*head, *body, _stream(a8)))
    return out


def _attn_geometry(q, k, v, out, batch, shared_kv, name):
    """Row strides, per-sample row counts and batch strides of an attention call.  shared_kv: k / v hold
    ONE key set ([Skv, ...] rows) that every batch sample attends to (batch strides 0)."""
    Mq, _, ldq = _rows(q, "q")
    Mk, _, ldk = _rows(k, "k")
    Mv, _, ldv = _rows(v, "v")
    Mo, _, ldo = _rows(out, "out")
    kb = 1 if shared_kv else batch
    if Mq % batch or Mk % kb or Mk != Mv or Mo != Mq:
        raise ValueError(f"{name}: row counts do not match batch")
    sq, skv = Mq // batch, Mk // kb
    bsk, bsv = (0, 0) if shared_kv else (skv * ldk, skv * ldv)
    return sq, skv, (ldq, ldk, ldv, ldo, sq * ldq, bsk, bsv, sq * ldo)


def attention(q, k, v, out, num_heads, batch, scale=None, shared_kv=False):
    """q/out: [batch*Sq, >=H*128] rows, k/v: [batch*Skv, ...] (views with row strides allowed);
    shared_kv: k/v are [Skv, ...], one key set for every sample."""
    sq, skv, strides = _attn_geometry(q, k, v, out, batch, shared_kv, "attention")
    hd = 128
    if scale is None:
        scale = hd ** -0.5
    _split_ws(0, q)
    _split_ws(4, q)
    _split_ws(5, q)             # the persistent grid's XCD item queues (zero-filled words)
    _lib.check(_lib.load().vs_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), batch, sq,
                                       skv, num_heads, hd, *strides, float(scale), _stream(q)))
    return out


def attention_add(q, k, v, out, num_heads, batch, scale=None, shared_kv=False):
    """out = bf16(out + bf16(attention(q, k, v))) in one launch (vs_attn_fwd_add: the checked kernel, at
    most 1984 keys); arguments as attention()."""
    sq, skv, strides = _attn_geometry(q, k, v, out, batch, shared_kv, "attention_add")
    hd = 128
    if scale is None:
        scale = hd ** -0.5
    _lib.check(_lib.load().vs_attn_fwd_add(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), batch, sq,
                                           skv, num_heads, hd, *strides, float(scale), _stream(q)))
    return out


def attention_split_plan(batch, sq, skv, heads, cus):
    """(whole-item workgroups, split tail items, pieces per item, tiles per piece) of vs_attn_fwd."""
    out = (ctypes.c_int * 4)()
    _lib.check(_lib.load().vs_attn_split_plan(batch, sq, skv, heads, cus, out))
    return tuple(out)


def gemm_split_plan(m, n, k, cus):
    """(whole-tile workgroups, split tail tiles, K pieces per tile, K per piece) of vs_gemm (256 schedule)."""
    out = (ctypes.c_int * 4)()
    _lib.check(_lib.load().vs_gemm_split_plan(m, n, k, cus, out))
    return tuple(out)


def layernorm_modulate(x, out, eps=1e-6, shift=None, scale=None, mod_bstride=0, rows_per_batch=0,
                       weight=None, bias=None):
    M, D, ldx = _rows(x, "x")
    Mo, Do, ldo = _rows(out, "out")
    if Mo != M or Do != D:
        raise ValueError("layernorm_modulate: shape mismatch")
    _lib.check(_lib.load().vs_layernorm_modulate(x.data_ptr(), ldx, out.data_ptr(), ldo, M, D, int(rows_per_batch),
                                                 _ptr(shift), _ptr(scale), int(mod_bstride), _ptr(weight),
                                                 _ptr(bias), float(eps), _stream(x)))
    return out


def layernorm_modulate_fp8(x, x8, qscale, eps=1e-6, shift=None, scale=None, mod_bstride=0, rows_per_batch=0,
                           weight=None, bias=None):
    """layernorm_modulate straight into fp8_linear's activation quantisation: x8 [M, D] uint8 (e4m3fn
    bytes), qscale [M] fp32 -- equal to quant_fp8_rows of layernorm_modulate's bf16 output."""
    M, D, ldx = _rows(x, "x")
    if x8.dtype != torch.uint8 or x8.dim() != 2 or x8.shape[0] != M or x8.shape[1] < D or x8.stride(1) != 1:
        raise ValueError("layernorm_modulate_fp8: x8 must be uint8 [M, >=D] with unit column stride")
    if qscale.dtype != torch.float32 or qscale.numel() < M or not qscale.is_contiguous():
        raise ValueError("layernorm_modulate_fp8: qscale must be contiguous float32 [M]")
    _lib.check(_lib.load().vs_layernorm_modulate_fp8(x.data_ptr(), ldx, x8.data_ptr(), x8.stride(0), qscale.data_ptr(),
                                                     M, D, int(rows_per_batch), _ptr(shift), _ptr(scale),
                                                     int(mod_bstride), _ptr(weight), _ptr(bias), float(eps),
                                                     _stream(x)))
    return x8, qscale


def layernorm_modulate_seg(x, out, seg_rows, eps=1e-6, shift=None, scale=None, mod_bstride=0, rows_per_batch=0,
                           weight=None, bias=None):
    """layernorm_modulate with two modulation rows per sample (vs_layernorm_modulate_seg): row r of
    sample b reads row 2 b + (r >= seg_rows) of shift / scale."""
    M, D, ldx = _rows(x, "x")
    Mo, Do, ldo = _rows(out, "out")
    if Mo != M or Do != D:
        raise ValueError("layernorm_modulate_seg: shape mismatch")
    _lib.check(_lib.load().vs_layernorm_modulate_seg(x.data_ptr(), ldx, out.data_ptr(), ldo, M, D,
                                                     int(rows_per_batch), int(seg_rows), _ptr(shift), _ptr(scale),
                                                     int(mod_bstride), _ptr(weight), _ptr(bias), float(eps),
                                                     _stream(x)))
    return out


def layernorm_modulate_fp8_seg(x, x8, qscale, seg_rows, eps=1e-6, shift=None, scale=None, mod_bstride=0,
                               rows_per_batch=0, weight=None, bias=None):
    """layernorm_modulate_fp8 with two modulation rows per sample (vs_layernorm_modulate_fp8_seg)."""
    M, D, ldx = _rows(x, "x")
    if x8.dtype != torch.uint8 or x8.dim() != 2 or x8.shape[0] != M or x8.shape[1] < D or x8.stride(1) != 1:
        raise ValueError("layernorm_modulate_fp8_seg: x8 must be uint8 [M, >=D] with unit column stride")
    if qscale.dtype != torch.float32 or qscale.numel() < M or not qscale.is_contiguous():
        raise ValueError("layernorm_modulate_fp8_seg: qscale must be contiguous float32 [M]")
    _lib.check(_lib.load().vs_layernorm_modulate_fp8_seg(x.data_ptr(), ldx, x8.data_ptr(), x8.stride(0),
                                                         qscale.data_ptr(), M, D, int(rows_per_batch), int(seg_rows),
                                                         _ptr(shift), _ptr(scale), int(mod_bstride), _ptr(weight),
                                                         _ptr(bias), float(eps), _stream(x)))
    return x8, qscale


def residual_layernorm(y, x, out, eps=1e-6, epilogue=VS_EPI_GATE_RES, gate=None, gate_bstride=0, gate_rows=0,
                       alpha=1.0, hint=None, hint_scale=1.0, shift=None, scale=None, mod_bstride=0,
                       rows_per_batch=0, weight=None, bias=None):
    """x = epilogue(y, x) (gate-residual / residual of a bf16 projection y the caller holds), then
    out = layernorm_modulate(x) -- one pass over the rows (vs_residual_layernorm).  A standalone fused
    row op of the ABI: the model does not call it, every GEMM of the model fuses its own epilogue."""
    M, D, ldy = _rows(y, "y")
    Mx, Dx, ldx = _rows(x, "x")
    Mo, Do, ldo = _rows(out, "out")
    if (Mx, Dx) != (M, D) or (Mo, Do) != (M, D):
        raise ValueError("residual_layernorm: shape mismatch")
    ep = _epilogue(None, None, gate, gate_bstride, hint, hint_scale, alpha, gate_rows)
    _lib.check(_lib.load().vs_residual_layernorm(y.data_ptr(), ldy, x.data_ptr(), ldx, out.data_ptr(), ldo, M, D,
                                                 int(epilogue), ep, int(rows_per_batch), _ptr(shift), _ptr(scale),
                                                 int(mod_bstride), _ptr(weight), _ptr(bias), float(eps), _stream(x)))
    return out


def rmsnorm_rope(x, weight, eps=1e-6, rope=None, grid=(1, 1, 1), rows_per_batch=0, token_offset=0, head_dim=128):
    M, D, ldx = _rows(x, "x")
    rlen = 0 if rope is None else rope.shape[0]
    if rope is not None and (rope.dtype != torch.float32 or rope.shape[1] != head_dim // 2 or rope.shape[2] != 2):
        raise ValueError("rope table must be float32 [len, head_dim/2, 2]")
    gf, gh, gw = grid
    _lib.check(_lib.load().vs_rmsnorm_rope(x.data_ptr(), ldx, M, D, head_dim, weight.data_ptr(), float(eps),
                                           _ptr(rope), rlen, gf, gh, gw, int(rows_per_batch), int(token_offset),
                                           _stream(x)))
    return x


def patchify(lat, out):
    _req(lat, "lat")
    B, C, T, H, W = lat.shape
    if not lat.is_contiguous() or not out.is_contiguous() or out.numel() != lat.numel():
        raise ValueError("patchify: contiguous tensors of equal numel required")
    _lib.check(_lib.load().vs_patchify(lat.data_ptr(), out.data_ptr(), B, C, T, H, W, _stream(lat)))
    return out


def patchify2(x, y, out):
    """out [B*S, ld] = im2col of cat([x, y], dim=1) for Conv3d k=s=(1,2,2), columns past 4(cx+cy) zero
    (vs_patchify2).  x [B or 1, cx, T, H, W], y [B or 1, cy, T, H, W] or None; a batch-1 operand is
    broadcast over out's B = rows / S."""
    _req(x, "x")
    if x.dim() != 5 or not x.is_contiguous():
        raise ValueError(f"x: expected a contiguous [B, C, T, H, W] tensor, got {tuple(x.shape)}")
    Bx, cx, T, H, W = x.shape
    By, cy = 1, 0
    if y is not None:
        _req(y, "y")
        if y.dim() != 5 or not y.is_contiguous() or tuple(y.shape[2:]) != (T, H, W) or y.device != x.device:
            raise ValueError(f"y: expected a contiguous [B, C, {T}, {H}, {W}] tensor on {x.device}, got {tuple(y.shape)}")
        By, cy = y.shape[0], y.shape[1]
    rows, cols, ld = _rows(out, "out")
    S = T * (H // 2) * (W // 2)
    if H % 2 or W % 2 or rows % S or cols != ld or cols < 4 * (cx + cy):
        raise ValueError(f"patchify2: out {tuple(out.shape)} does not hold {S}-token samples of {4 * (cx + cy)} columns")
    B = rows // S
    if Bx not in (1, B) or By not in (1, B):
        raise ValueError(f"patchify2: batch {Bx} / {By} against {B} output samples")
    _lib.check(_lib.load().vs_patchify2(x.data_ptr(), 0 if Bx == 1 and B > 1 else cx * T * H * W, cx, _ptr(y),
                                        0 if By == 1 and B > 1 else cy * T * H * W, cy, out.data_ptr(), ld, B, T, H, W,
                                        _stream(x)))
    return out


def gelu_erf(x, out=None):
    """out = bf16(gelu(x)) with the erf form of nn.GELU() (vs_gelu_erf); in place by default."""
    _req(x, "x")
    out = x if out is None else _req(out, "out")
    if not x.is_contiguous() or not out.is_contiguous() or out.numel() != x.numel():
        raise ValueError("gelu_erf: contiguous tensors of equal numel required")
    _lib.check(_lib.load().vs_gelu_erf(x.data_ptr(), out.data_ptr(), x.numel(), _stream(x)))
    return out


def unpatchify(tokens, out):
    _req(out, "out")
    B, C, T, H, W = out.shape
    if not tokens.is_contiguous() or not out.is_contiguous() or out.numel() != tokens.numel():
        raise ValueError("unpatchify: contiguous tensors of equal numel required")
    _lib.check(_lib.load().vs_unpatchify(tokens.data_ptr(), out.data_ptr(), B, C, T, H, W, _stream(out)))
    return out


def unpatchify_skip(tokens, out, skip):
    """unpatchify whose sample b reads its S rows behind `skip` prepended ones: tokens is
    [B * (skip + S), 4 C] (vs_unpatchify_skip; skip 0 is unpatchify)."""
    _req(out, "out"), _req(tokens, "tokens")
    B, C, T, H, W = out.shape
    S = T * (H // 2) * (W // 2)
    if skip < 0 or not tokens.is_contiguous() or not out.is_contiguous() or tokens.dim() != 2 or \
            tuple(tokens.shape) != (B * (skip + S), 4 * C):
        raise ValueError(f"unpatchify_skip: tokens {tuple(tokens.shape)} are not [{B} * ({skip} + {S}), {4 * C}]")
    _lib.check(_lib.load().vs_unpatchify_skip(tokens.data_ptr(), out.data_ptr(), B, C, T, H, W, int(skip),
                                              _stream(out)))
    return out


def ref_rows(src, dst, batch, n, s):
    """dst [batch * (n + s), D]: the first n rows of every sample = src's ([n, D]: one set for all, or
    [batch * n, D]); no other row is written (vs_ref_rows)."""
    Ms, D, lds = _rows(src, "src")
    Md, Dd, ldd = _rows(dst, "dst")
    if Dd != D or lds != D or Ms not in (n, batch * n) or Md != batch * (n + s):
        raise ValueError(f"ref_rows: src {tuple(src.shape)} / dst {tuple(dst.shape)} against batch {batch}, "
                         f"{n} + {s} rows")
    _lib.check(_lib.load().vs_ref_rows(src.data_ptr(), 0 if Ms == n and batch > 1 else n * D, dst.data_ptr(), ldd,
                                       batch, n, s, D, _stream(dst)))
    return dst


def camera_rays(intrinsics, c2w, out):
    """out bf16 [24, T, H, W]: the Pluecker rays of the pixel frames, grouped in fours
    (vs_camera_rays).  intrinsics fp32 [F, 4], c2w fp32 [F, 3, 4], F >= 4 T - 3."""
    _req(out, "out")
    if out.dim() != 4 or out.shape[0] != 24 or not out.is_contiguous():
        raise ValueError(f"camera_rays: out must be a contiguous [24, T, H, W] tensor, got {tuple(out.shape)}")
    F = intrinsics.shape[0]
    for t, name, shape in ((intrinsics, "intrinsics", (F, 4)), (c2w, "c2w", (F, 3, 4))):
        if t.dtype != torch.float32 or t.device != out.device or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"camera_rays: {name} must be contiguous float32 {shape} on {out.device}")
    _, T, H, W = out.shape
    if F < 4 * T - 3:
        raise ValueError(f"camera_rays: {F} pixel frames for {T} latent frames (at least {4 * T - 3})")
    _lib.check(_lib.load().vs_camera_rays(intrinsics.data_ptr(), c2w.data_ptr(), out.data_ptr(), F, T, H, W,
                                          _stream(out)))
    return out


def camera_im2col(x, out):
    """x [C, T, H, W] -> out [T (H/16) (W/16), 256 C]: PixelUnshuffle(8) + the 2x2 / stride 2 unfold
    (vs_camera_im2col)."""
    _req(x, "x")
    if x.dim() != 4 or not x.is_contiguous() or x.shape[2] % 16 or x.shape[3] % 16:
        raise ValueError(f"camera_im2col: x must be a contiguous [C, T, H, W] tensor with H, W multiples of 16, "
                         f"got {tuple(x.shape)}")
    C, T, H, W = x.shape
    rows, cols, ldo = _rows(out, "out")
    if rows != T * (H // 16) * (W // 16) or cols != 256 * C:
        raise ValueError(f"camera_im2col: out {tuple(out.shape)} is not [{T * (H // 16) * (W // 16)}, {256 * C}]")
    _lib.check(_lib.load().vs_camera_im2col(x.data_ptr(), out.data_ptr(), ldo, C, T, H, W, _stream(x)))
    return out


def relu(x):
    """x = max(x, 0) in place (vs_relu)."""
    _req(x, "x")
    if not x.is_contiguous() or x.numel() % 8:
        raise ValueError("relu: a contiguous tensor of a multiple of 8 elements required")
    _lib.check(_lib.load().vs_relu(x.data_ptr(), x.numel(), _stream(x)))
    return x


def face_attn(q, k, v, wq, out=None, *, batch, num_heads, frames, tokens_per_frame, nkeys, token_offset=0,
              eps=1e-6, scale=None, head_dim=128):
    """FaceBlock's attention (vs_face_attn): q [batch * rows_per_batch, >= H*128] rows, each attending the
    nkeys keys of its latent frame with the per-head RMSNorm of q (weight wq [128]) fused in.  k, v:
    [batch or 1, frames * nkeys, >= H*128] views sharing one row and one sample stride (k normalised by
    head_rmsnorm).  out defaults to q (in place)."""
    M, Dq, ldq = _rows(q, "q")
    out = q if out is None else out
    Mo, Do, ldo = _rows(out, "out")
    width = num_heads * head_dim
    if M % batch or Mo != M or Dq < width or Do < width:
        raise ValueError(f"face_attn: q {tuple(q.shape)} / out {tuple(out.shape)} against batch {batch}, "
                         f"{num_heads} heads")
    _req(k, "k"), _req(v, "v"), _req(wq, "wq")
    if k.dim() != 3 or k.shape != v.shape or k.stride() != v.stride() or k.stride(2) != 1 or \
            k.shape[0] not in (1, batch) or k.shape[1] != frames * nkeys or k.shape[2] < width:
        raise ValueError(f"face_attn: k {tuple(k.shape)} / v {tuple(v.shape)} are not [{batch} or 1, "
                         f"{frames} * {nkeys}, >= {width}] views of one layout")
    if wq.numel() != head_dim or not wq.is_contiguous():
        raise ValueError(f"face_attn: wq must be contiguous [{head_dim}]")
    kv_bs = 0 if k.shape[0] == 1 else k.stride(0)
    sc = head_dim ** -0.5 if scale is None else scale
    _lib.check(_lib.load().vs_face_attn(q.data_ptr(), ldq, k.data_ptr(), v.data_ptr(), k.stride(1), kv_bs,
                                        out.data_ptr(), ldo, wq.data_ptr(), batch, M // batch, num_heads, head_dim,
                                        frames, tokens_per_frame, nkeys, int(token_offset), float(eps), float(sc),
                                        _stream(q)))
    return out


def head_rmsnorm(x, weight, num_heads, eps=1e-6, head_dim=128):
    """The reference RMSNorm over each 128-wide head of every row of x, in place (vs_head_rmsnorm)."""
    M, D, ldx = _rows(x, "x")
    _req(weight, "weight")
    if D < num_heads * head_dim or weight.numel() != head_dim or not weight.is_contiguous():
        raise ValueError(f"head_rmsnorm: x {tuple(x.shape)} / weight {tuple(weight.shape)} against {num_heads} heads "
                         f"of {head_dim}")
    _lib.check(_lib.load().vs_head_rmsnorm(x.data_ptr(), ldx, M, num_heads, head_dim, weight.data_ptr(), float(eps),
                                           _stream(x)))
    return x


def ln_silu(x, out=None, eps=1e-6, norm=True):
    """out = bf16(silu(bf16(LayerNorm(x)))) without affine (vs_ln_silu); norm=False: SiLU alone.  In place
    by default."""
    M, D, ldx = _rows(x, "x")
    out = x if out is None else out
    Mo, Do, ldo = _rows(out, "out")
    if (Mo, Do) != (M, D):
        raise ValueError("ln_silu: shape mismatch")
    _lib.check(_lib.load().vs_ln_silu(x.data_ptr(), ldx, out.data_ptr(), ldo, M, D, int(bool(norm)), float(eps),
                                      _stream(x)))
    return out


def _frames(t, name, c=None):
    """(n, H, W, frame stride, pixel stride) of a channels-last [n, H, W, >= c] bf16 view whose pixels of a
    frame are evenly spaced (include/vstyler_motion.h: frames ns apart, pixels ld apart)."""
    _req(t, name)
    if t.dim() != 4 or t.stride(3) != 1 or t.stride(1) != t.shape[2] * t.stride(2):
        raise ValueError(f"{name}: expected a channels-last [n, H, W, C] view with evenly spaced pixels, got "
                         f"{tuple(t.shape)} strides {tuple(t.stride())}")
    if c is not None and t.shape[3] != c:
        raise ValueError(f"{name}: expected {c} channels, got {t.shape[3]}")
    return t.shape[0], t.shape[1], t.shape[2], t.stride(0), t.stride(2)


def motion_stem(frames, weight, bias, out):
    """The motion encoder's stem (vs_motion_stem): frames uint8 [n, H, W, 3] or bf16 planar [3, n, H, W];
    weight bf16 [c0, 3] (prepared), bias bf16 [c0]; out channels-last [n, H, W, c0]."""
    n, H, W, ns, ld = _frames(out, "out")
    c0 = out.shape[3]
    u8 = frames.dtype == torch.uint8
    want = (n, H, W, 3) if u8 else (3, n, H, W)
    if frames.dtype not in (torch.uint8, BF16) or not frames.is_cuda or not frames.is_contiguous() or \
            tuple(frames.shape) != want:
        raise ValueError(f"motion_stem: frames must be contiguous uint8 [n, H, W, 3] or bfloat16 [3, n, H, W] on the "
                         f"device matching out {tuple(out.shape)}, got {tuple(frames.shape)} {frames.dtype}")
    _req(weight, "weight"), _req(bias, "bias")
    if tuple(weight.shape) != (c0, 3) or not weight.is_contiguous() or bias.numel() != c0 or not bias.is_contiguous():
        raise ValueError(f"motion_stem: weight {tuple(weight.shape)} / bias {tuple(bias.shape)} against {c0} channels")
    _lib.check(_lib.load().vs_motion_stem(frames.data_ptr(), int(u8), weight.data_ptr(), bias.data_ptr(),
                                          out.data_ptr(), ns, ld, n, H, W, c0, _stream(out)))
    return out


def lrelu_blur(x, out, bias=None, pad=(2, 2), step=1):
    """out = Blur(pad)(ACT(x, bias))[::step, ::step] (vs_lrelu_blur; bias None: the blur alone).  x [n, H, W, C],
    out [n, ceil((H + p0 + p1 - 3) / step), ceil((W + p0 + p1 - 3) / step), C], channels-last views."""
    n, H, W, xns, ldx = _frames(x, "x")
    c = x.shape[3]
    no, Ho, Wo, yns, ldy = _frames(out, "out", c)
    p0, p1 = pad
    if step not in (1, 2) or (no, Ho, Wo) != (n, -(-(H + p0 + p1 - 3) // step), -(-(W + p0 + p1 - 3) // step)):
        raise ValueError(f"lrelu_blur: out {tuple(out.shape)} against x {tuple(x.shape)}, pad {pad}, step {step}")
    if bias is not None and (_req(bias, "bias").numel() != c or not bias.is_contiguous()):
        raise ValueError(f"lrelu_blur: bias {tuple(bias.shape)} against {c} channels")
    _lib.check(_lib.load().vs_lrelu_blur(x.data_ptr(), xns, ldx, out.data_ptr(), yns, ldy, _ptr(bias), n, H, W, c,
                                         int(p0), int(p1), int(step), _stream(x)))
    return out


def lrelu_merge(x, bias, skip=None, out=None):
    """out = ACT(x, bias), with skip: bf16(bf16(ACT(x, bias) + skip) / sqrt(2)) (vs_lrelu_merge).  Channels-last
    [n, H, W, C] views; in place on x by default."""
    n, H, W, xns, ldx = _frames(x, "x")
    c = x.shape[3]
    out = x if out is None else out
    geo = _frames(out, "out", c)
    sns = lds = 0
    if skip is not None:
        sgeo = _frames(skip, "skip", c)
        if sgeo[:3] != (n, H, W):
            raise ValueError(f"lrelu_merge: skip {tuple(skip.shape)} against x {tuple(x.shape)}")
        sns, lds = sgeo[3], sgeo[4]
    if geo[:3] != (n, H, W) or _req(bias, "bias").numel() != c or not bias.is_contiguous():
        raise ValueError(f"lrelu_merge: out {tuple(out.shape)} / bias {tuple(bias.shape)} against x {tuple(x.shape)}")
    _lib.check(_lib.load().vs_lrelu_merge(x.data_ptr(), xns, ldx, bias.data_ptr(), _ptr(skip), sns, lds,
                                          out.data_ptr(), geo[3], geo[4], n, H * W, c, _stream(x)))
    return out


def motion_direction(alpha, q, out):
    """out[t, j] = bf16(sum_i bf16(alpha[t, i] q[j, i])) (vs_motion_direction): alpha [T, m], q [d, m], out [T, d]."""
    T, m, lda = _rows(alpha, "alpha")
    d, mq, ldq = _rows(q, "q")
    To, do, ldo = _rows(out, "out")
    if mq != m or (To, do) != (T, d):
        raise ValueError(f"motion_direction: alpha {tuple(alpha.shape)} / q {tuple(q.shape)} / out {tuple(out.shape)}")
    _lib.check(_lib.load().vs_motion_direction(alpha.data_ptr(), lda, q.data_ptr(), ldq, out.data_ptr(), ldo, T, d, m,
                                               _stream(out)))
    return out


def cfg_euler(v_pos, v_neg, x, cfg_scale, dsigma):
    for t, n in ((v_pos, "v_pos"), (x, "x")):
        _req(t, n)
        if not t.is_contiguous():
            raise ValueError(f"{n} must be contiguous")
    use_cfg = v_neg is not None
    _lib.check(_lib.load().vs_cfg_euler(v_pos.data_ptr(), _ptr(v_neg), x.data_ptr(), x.numel(), float(cfg_scale),
                                        float(dsigma), int(use_cfg), _stream(x)))
    return x


def cfg_euler_dev(v_pos, v_neg, x, cfg_scale, dsigma_dev):
    """cfg_euler with dsigma read from a one-element fp32 device tensor (graph-replayable)."""
    for t, n in ((v_pos, "v_pos"), (x, "x")):
        _req(t, n)
        if not t.is_contiguous():
            raise ValueError(f"{n} must be contiguous")
    if dsigma_dev.dtype != torch.float32 or not dsigma_dev.is_cuda:
        raise ValueError("dsigma_dev must be a float32 device tensor")
    _lib.check(_lib.load().vs_cfg_euler_dev(v_pos.data_ptr(), _ptr(v_neg), x.data_ptr(), x.numel(), float(cfg_scale),
                                            dsigma_dev.data_ptr(), int(v_neg is not None), _stream(x)))
    return x


def flow_add_noise(x0, noise, sigma, out=None):
    """(1 - sigma) * x0 + sigma * noise (vs_flow_add_noise): bf16 tensors with torch's bf16 rounding
    points (flow_match.py:99), fp32 tensors op by op (fm_solvers_unipc.py:797-799).  out may be x0
    or noise; a new tensor by default."""
    if x0.dtype != noise.dtype or x0.dtype not in (BF16, torch.float32):
        raise ValueError(f"flow_add_noise: x0 / noise must both be bfloat16 or both float32, got "
                         f"{x0.dtype} / {noise.dtype}")
    if out is None:
        out = torch.empty_like(x0)
    for t, n in ((x0, "x0"), (noise, "noise"), (out, "out")):
        if not t.is_cuda or t.device != x0.device:
            raise ValueError(f"{n}: expected a tensor on {x0.device}")
        if t.dtype != x0.dtype or t.shape != x0.shape:
            raise ValueError(f"{n}: expected {tuple(x0.shape)} {x0.dtype}, got {tuple(t.shape)} {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{n} must be contiguous")
    _lib.check(_lib.load().vs_flow_add_noise(x0.data_ptr(), noise.data_ptr(), out.data_ptr(), x0.numel(),
                                             float(sigma), int(x0.dtype == torch.float32), _stream(x0)))
    return out


def _bcthw(t, name):
    _req(t, name)
    if t.dim() != 5 or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous [B, C, T, H, W] tensor, got {tuple(t.shape)}")
    return t


def _frame_vec(v, n, like, name):
    if v.dtype != BF16 or v.device != like.device or v.dim() != 1 or v.shape[0] != n or not v.is_contiguous():
        raise ValueError(f"{name}: expected {n} contiguous bfloat16 elements on {like.device}")
    return v


def window_gather(src, t0, dst):
    """dst[B, C, L, H, W] = src[:, :, t0:t0 + L] (vs_vae_copy_frames: one strided copy, no allocation)."""
    _bcthw(src, "src"), _bcthw(dst, "dst")
    B, C, T, H, W = src.shape
    L = dst.shape[2]
    if dst.shape != (B, C, L, H, W) or t0 < 0 or t0 + L > T:
        raise ValueError(f"window_gather: frames [{t0}, {t0 + L}) of {tuple(src.shape)} into {tuple(dst.shape)}")
    plane = H * W
    _lib.check(_lib.load().vs_vae_copy_frames(src.data_ptr() + 2 * t0 * plane, T * plane, dst.data_ptr(), L * plane,
                                              B * C, L * plane, _stream(src)))
    return dst


def window_blend(out, mask, value, t0):
    """value[:, :, t0:t0 + L] += out * mask in the reference's bf16 arithmetic (vs_window_blend);
    out [B, C, L, H, W], mask [L], value [B, C, T, H, W]."""
    _bcthw(out, "out"), _bcthw(value, "value")
    B, C, T, H, W = value.shape
    L = out.shape[2]
    if out.shape != (B, C, L, H, W) or out.device != value.device:
        raise ValueError(f"window_blend: out {tuple(out.shape)} does not match value {tuple(value.shape)}")
    _frame_vec(mask, L, value, "mask")
    _lib.check(_lib.load().vs_window_blend(out.data_ptr(), mask.data_ptr(), value.data_ptr(), B * C, T, L, int(t0),
                                           H * W, _stream(value)))
    return value


def window_finish(value, weight, out=None):
    """value / weight[T] in bf16 (vs_window_finish), in place by default."""
    _bcthw(value, "value")
    out = value if out is None else _bcthw(out, "out")
    B, C, T, H, W = value.shape
    if out.shape != value.shape or out.device != value.device:
        raise ValueError(f"window_finish: out {tuple(out.shape)} does not match value {tuple(value.shape)}")
    _frame_vec(weight, T, value, "weight")
    _lib.check(_lib.load().vs_window_finish(value.data_ptr(), weight.data_ptr(), out.data_ptr(), B * C, T, H * W,
                                            _stream(value)))
    return out


def resize_nearest_u8(frames, height, width, out=None):
    """(T, H, W, 3) uint8 device frames -> (T, height, width, 3) uint8, nearest neighbour with
    F.interpolate(mode="nearest")'s source index (vs_resize_nearest_u8).  out: a contiguous uint8
    tensor of that shape (any alignment), allocated when None."""
    if frames.dtype != torch.uint8 or not frames.is_cuda or frames.dim() != 4 or not frames.is_contiguous():
        raise ValueError(f"frames must be a contiguous (T, H, W, 3) uint8 device tensor, got "
                         f"{tuple(frames.shape)} {frames.dtype}")
    T, H, W, C = frames.shape
    if out is None:
        out = torch.empty((T, int(height), int(width), C), dtype=torch.uint8, device=frames.device)
    elif out.dtype != torch.uint8 or out.device != frames.device or not out.is_contiguous() or \
            tuple(out.shape) != (T, int(height), int(width), C):
        raise ValueError(f"out must be a contiguous uint8 tensor {(T, int(height), int(width), C)} on "
                         f"{frames.device}, got {tuple(out.shape)} {out.dtype}")
    _lib.check(_lib.load().vs_resize_nearest_u8(frames.data_ptr(), out.data_ptr(), T, H, W, int(height), int(width),
                                                C, _stream(frames)))
    return out


def time_sinusoid(t, out):
    _lib.check(_lib.load().vs_time_sinusoid(t.data_ptr(), out.data_ptr(), t.numel(), out.shape[-1], _stream(t)))
    return out


def mod_add(param, tv, out, tv_bstride, tv_rstride):
    """out[b][r][d] = bf16(param[r][d] + tv[b*bs + r*rs + d]); out is [B, R, D] contiguous."""
    B, R, D = out.shape
    _lib.check(_lib.load().vs_mod_add(param.data_ptr(), tv.data_ptr(), out.data_ptr(), B, R, D, int(tv_bstride),
                                      int(tv_rstride), _stream(out)))
    return out


def axpy(x, y, scale):
    _lib.check(_lib.load().vs_axpy(x.data_ptr(), y.data_ptr(), float(scale), x.numel(), _stream(x)))
    return x


def ulysses_permute(src, dst, batch, s_local, world, cols_per_rank, ld_local, jstride, mode, packed_ld=None):
    """Row permutation between token-sharded / all_to_all-packed / head-sharded layouts (packed rows
    packed_ld elements apart, default cols_per_rank)."""
    pld = cols_per_rank if packed_ld is None else packed_ld
    _lib.check(_lib.load().vs_ulysses_permute_rows(src.data_ptr(), dst.data_ptr(), int(batch), int(s_local),
                                                   int(world), int(cols_per_rank), int(ld_local), int(jstride),
                                                   int(pld), int(mode), _stream(src)))
    return dst


__all__ = ["set_option", "get_option", "options", "ulysses_permute", "gemm", "attention", "attention_add", "patchify2", "gelu_erf", "layernorm_modulate", "rmsnorm_rope", "patchify", "unpatchify", "cfg_euler", "flow_add_noise",
           "window_gather", "window_blend", "window_finish",
           "time_sinusoid", "mod_add", "axpy", "VS_EPI_BIAS", "VS_EPI_GELU", "VS_EPI_SILU", "VS_EPI_GATE_RES",
           "VS_EPI_RES"]
