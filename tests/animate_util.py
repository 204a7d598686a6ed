"""Test-side restatement of Wan2.2-Animate (diffsynth/models/wan_video_animate_adapter.py: FaceEncoder,
FaceBlock, WanAnimateAdapter.after_patch_embedding / after_transformer_block) and the references of the three
kernels of include/vstyler_animate.h.  Model restatements follow the oracle's convention (O.ACC_DTYPE
accumulation, a bf16 rounding wherever the reference's bf16 modules materialise a tensor) and are composed
from oracle.wan_oracle and tests/i2v_util.py; the kernel references are float64 with the kernels' rounding
points.  Everything runs on CPU tensors.  Never used by the product path."""
import math

import torch
import torch.nn.functional as F

import gpu_util as U
import i2v_util as I
from oracle import wan_oracle as O

BF16 = torch.bfloat16
HD = 128
EPS = 1e-6


# ------------------------------------------------------------------------------------------ tiny weights
def tiny_cfg(num_layers=6):
    """The tiny I2V DiT of tests/test_i2v_gpu.py (dim 256, 2 heads, in_dim 36, image input) with 6 layers:
    fuser blocks after blocks 0 and 5."""
    return I.tiny_cfg(num_layers=num_layers, has_image_input=True)


def adapter_param_shapes(dim, num_heads, num_layers, in_dim=512, enc_heads=4):
    """The 75 parameters of WanAnimateAdapter outside motion_encoder (wan_video_animate_adapter.py:615-621)
    at any width: 2 + 8 per fuser block + 9."""
    s = {"pose_patch_embedding.weight": (dim, 16, 1, 2, 2), "pose_patch_embedding.bias": (dim,)}
    for i in range(-(-num_layers // 5)):
        p = f"face_adapter.fuser_blocks.{i}."
        s[p + "linear1_kv.weight"], s[p + "linear1_kv.bias"] = (2 * dim, dim), (2 * dim,)
        s[p + "linear1_q.weight"], s[p + "linear1_q.bias"] = (dim, dim), (dim,)
        s[p + "linear2.weight"], s[p + "linear2.bias"] = (dim, dim), (dim,)
        s[p + "q_norm.weight"], s[p + "k_norm.weight"] = (HD,), (HD,)
    e = "face_encoder."
    s[e + "conv1_local.conv.weight"], s[e + "conv1_local.conv.bias"] = (1024 * enc_heads, in_dim, 3), (1024 * enc_heads,)
    for n in ("conv2", "conv3"):
        s[e + n + ".conv.weight"], s[e + n + ".conv.bias"] = (1024, 1024, 3), (1024,)
    s[e + "out_proj.weight"], s[e + "out_proj.bias"] = (dim, 1024), (dim,)
    s[e + "padding_tokens"] = (1, 1, 1, dim)
    return s


def adapter_weights(dim, num_heads, num_layers, in_dim=512, seed=31):
    """Seeded bf16 weights by the oracle's init rule (norm weights 1 + 0.1 N, biases 0.01 N, the rest
    N(0, 0.02)); the convolutions of the face encoder at N(0, 0.02) too; linear2 times 8 (exact in bf16) so
    the adapter's residual is not lost beside the stream."""
    gen = torch.Generator("cpu").manual_seed(seed)
    W = {}
    for k, shape in adapter_param_shapes(dim, num_heads, num_layers, in_dim).items():
        W[k] = O.init_weight(k, shape, gen, dim)
        if k.endswith("linear2.weight"):
            W[k] = (W[k].float() * 8).to(BF16)
    return W


def build_adapter(W, dim, num_heads, num_layers, in_dim=512, device="cuda"):
    from vstyler.models import WanAnimateAdapter
    a = WanAnimateAdapter(dim=dim, num_heads=num_heads, num_layers=num_layers, in_dim=in_dim, device=device)
    a.load_state_dict(W, strict=True)
    return a


def animate_inputs(T=3, h=8, w=12, t_face=5, in_dim=512, seed=23, batch=1):
    """pose_latents (1, 16, T - 1, h, w) ~ N(0, 1) and face motion (batch, t_face, in_dim) ~ N(0, 1), bf16."""
    g = torch.Generator("cpu").manual_seed(seed)
    pose = torch.randn((1, 16, T - 1, h, w), generator=g).to(BF16)
    motion = torch.randn((batch, t_face, in_dim), generator=g).to(BF16)
    return pose, motion


# ----------------------------------------------------------------------------- the model's restatements
# PURE: every rounding point off and every operation in float64 -- the arithmetic of the float64 reference
# modules that tests/golden/make_animate_ref.py records (tests/test_animate_cpu.py holds the restatement
# against that fixture in this mode).
PURE = False


def pure_float64(fn):
    """fn() with the adapter's restatements in float64 throughout and no bf16 rounding."""
    global PURE
    old, PURE = PURE, True
    try:
        return I.with_float64(fn)
    finally:
        PURE = old


def _bf(x):
    return x if PURE else O.bf(x)


def _acc(x):
    return x.to(torch.float64 if PURE else O.ACC_DTYPE)


def linear(x, w, b):
    """nn.Linear in bf16: accumulation in O.ACC_DTYPE, + bias, one rounding."""
    return _bf(_acc(x) @ _acc(w).t() + _acc(b))


def layer_norm(x, eps=EPS):
    """nn.LayerNorm without affine on a bf16 tensor: fp32 statistics, one rounding."""
    xf = x.double() if PURE else x.float()
    return _bf(F.layer_norm(xf, (x.shape[-1],), None, None, eps))


def causal_conv1d(x, w, b, stride):
    """CausalConv1d.forward (:61-63) on [B, C, T]: two replicate-padded frames in front, Conv1d, one rounding."""
    xp = F.pad(_acc(x), (2, 0), mode="replicate")
    return _bf(F.conv1d(xp, _acc(w), _acc(b), stride=stride))


def silu(x):
    return _bf(F.silu(x.to(torch.float64)))


def face_encoder(motion, W, num_heads=4, p="face_encoder."):
    """FaceEncoder.forward (:88-114): [B, T, C] -> [B, T', num_heads + 1, hidden]."""
    b = motion.shape[0]
    x = causal_conv1d(motion.transpose(1, 2), W[p + "conv1_local.conv.weight"], W[p + "conv1_local.conv.bias"], 1)
    x = x.view(b, num_heads, -1, x.shape[-1]).flatten(0, 1).transpose(1, 2)          # "b (n c) t -> (b n) t c"
    x = silu(layer_norm(x))
    for n in ("conv2", "conv3"):
        x = causal_conv1d(x.transpose(1, 2), W[p + n + ".conv.weight"], W[p + n + ".conv.bias"], 2).transpose(1, 2)
        x = silu(layer_norm(x))
    x = linear(x, W[p + "out_proj.weight"], W[p + "out_proj.bias"])
    x = x.view(b, num_heads, x.shape[1], x.shape[2]).transpose(1, 2)                 # "(b n) t c -> b t n c"
    pad = W[p + "padding_tokens"].to(x.dtype).expand(b, x.shape[1], 1, x.shape[3])
    return torch.cat([x, pad], dim=2)


def motion_tokens(motion, W):
    """after_patch_embedding (:638-642): the face encoder's tokens behind a zero frame."""
    m = face_encoder(motion, W)
    return torch.cat([torch.zeros_like(m[:, :1]), m], dim=1)


def head_rms_norm(x, weight, heads, eps=EPS):
    """RMSNorm (:145-172) over each head's 128 columns: fp32 norm, cast bf16, times the bf16 weight."""
    shp = x.shape
    xf = x.reshape(*shp[:-1], heads, HD).float()        # _norm(x.float()): fp32 also under a float64 module
    n = _bf(xf * torch.rsqrt(xf.pow(2).mean(dim=-1, keepdim=True) + eps))
    if PURE:                                            # .type_as(x), then the weight, in the module's float64
        return (n.double() * weight.double()).reshape(shp)
    return _bf(n.float() * weight.float()).reshape(shp)


def face_attention(q, k, v, heads, frames):
    """The rearranges and the scaled_dot_product_attention of FaceBlock.forward (:296-303): every frame's
    tokens against that frame's N keys.  q [B, S, D] (normalised), k, v [B, frames, N, D]."""
    B, S, D = q.shape
    hw = S // frames
    qf = _acc(q.reshape(B, frames, hw, heads, HD).permute(0, 1, 3, 2, 4))                  # B L H S D
    kf = _acc(k.reshape(B, frames, -1, heads, HD).permute(0, 1, 3, 2, 4))                  # B L H N D
    vf = _acc(v.reshape(B, frames, -1, heads, HD).permute(0, 1, 3, 2, 4))
    p = torch.softmax(qf @ kf.transpose(-1, -2) * HD ** -0.5, dim=-1)
    return _bf((p @ vf).permute(0, 1, 3, 2, 4).reshape(B, S, D))


def face_block(x, motion_vec, W, p, heads):
    """FaceBlock.forward (:272-310) without a motion mask: the residual `output`."""
    D = x.shape[-1]
    kv = linear(layer_norm(motion_vec), W[p + "linear1_kv.weight"], W[p + "linear1_kv.bias"])
    q = linear(layer_norm(x), W[p + "linear1_q.weight"], W[p + "linear1_q.bias"])
    k, v = kv[..., :D], kv[..., D:]
    q = head_rms_norm(q, W[p + "q_norm.weight"], heads)
    k = head_rms_norm(k, W[p + "k_norm.weight"], heads)
    o = face_attention(q, k, v, heads, motion_vec.shape[1])
    return linear(o, W[p + "linear2.weight"], W[p + "linear2.bias"])


def model_fn(W, A, cfg, latents, timestep, context, y=None, clip_feature=None, pose_latents=None, motion=None):
    """i2v_util.model_fn with the adapter (weights A): after_patch_embedding's x[:, :, 1:] += pose (a bf16
    add on the latent frames 1..) and after_transformer_block's x = FaceBlock(x, motion_vec) + x after every
    fifth block.  motion [1 or B, T_face, C]: one set of motion vectors per CFG sample."""
    D, H, eps = cfg["dim"], cfg["num_heads"], cfg["eps"]
    B = context.shape[0]
    t, t_mod = O.time_embed(timestep.expand(B) if timestep.shape[0] != B else timestep, W, D)
    ctx = O.text_embed(context, W)
    x = latents.expand(B, *latents.shape[1:]) if latents.shape[0] != B else latents
    if y is not None:
        x = torch.cat([x, y.expand(B, *y.shape[1:])], dim=1)
    image = bool(cfg.get("has_image_input")) and clip_feature is not None
    if image:
        emb = I.img_emb(clip_feature, W, cfg)
        ctx = torch.cat([emb.expand(B, *emb.shape[1:]), ctx], dim=1)
    x, (f, h, w) = O.patchify(x, W["patch_embedding.weight"], W["patch_embedding.bias"])
    if pose_latents is not None:
        pose, _ = O.patchify(pose_latents, A["pose_patch_embedding.weight"], A["pose_patch_embedding.bias"])
        x = torch.cat([x[:, :h * w], O.add(x[:, h * w:], pose.expand(B, *pose.shape[1:]))], dim=1)
    mv = None
    if motion is not None:
        mv = motion_tokens(motion, A)
        mv = mv.expand(B, *mv.shape[1:]) if mv.shape[0] != B else mv
    freqs = O.rope_freqs(f, h, w, D // H)
    for i in range(cfg["num_layers"]):
        x = I.dit_block(x, ctx, t_mod, freqs, W, f"blocks.{i}.", H, image, eps)
        if mv is not None and i % 5 == 0:
            x = O.add(face_block(x, mv, A, f"face_adapter.fuser_blocks.{i // 5}.", H), x)
    x = O.head(x, t, W, eps)
    return O.unpatchify(x, (f, h, w), cfg["out_dim"])


# ---------------------------------------------------------------------- the y of WanVideoPostUnit_AnimateInpaint
def get_i2v_mask(lat_t, lat_h, lat_w, mask_len=1, mask_pixel_values=None):
    """wan_video_new.py:1118-1127, literally."""
    if mask_pixel_values is None:
        msk = torch.zeros(1, (lat_t - 1) * 4 + 1, lat_h, lat_w)
    else:
        msk = mask_pixel_values.clone()
    msk[:, :mask_len] = 1
    msk = torch.concat([torch.repeat_interleave(msk[:, 0:1], repeats=4, dim=1), msk[:, 1:]], dim=1)
    msk = msk.view(1, msk.shape[1] // 4, 4, lat_h, lat_w)
    msk = msk.transpose(1, 2)[0]
    return msk


def inpaint_y(ref_latents, bg_latents, mask_pixels):
    """wan_video_new.py:1129-1151 from the encoded tensors: ref_latents (16, 1, h, w) of input_image,
    bg_latents (16, T, h, w) of the inpaint video, mask_pixels (1, 1, F, H, W) in [0, 1] (the preprocessed
    mask video).  Returns y (1, 20, 1 + T, h, w) bf16."""
    _, lat_t, lat_h, lat_w = bg_latents.shape
    y_ref = torch.concat([get_i2v_mask(1, lat_h, lat_w, 1), ref_latents.float()]).to(BF16)
    m = 1 - mask_pixels
    m = m.permute(0, 2, 1, 3, 4).flatten(0, 1)                                   # "b c t h w -> (b t) c h w"
    m = F.interpolate(m, size=(lat_h, lat_w), mode="nearest")
    m = m.view(1, -1, m.shape[1], lat_h, lat_w)[:, :, 0]                         # "(b t) c h w -> b t c h w"[:, :, 0]
    msk_reft = get_i2v_mask(lat_t, lat_h, lat_w, 0, mask_pixel_values=m)
    y_reft = torch.concat([msk_reft, bg_latents.float()]).to(BF16)
    return torch.concat([y_ref, y_reft], dim=1).unsqueeze(0)


# ------------------------------------------------------------------- vs_head_rmsnorm / vs_ln_silu references
ROW_SHAPES = [(rows, heads) for rows in (1, 5) for heads in (1, 40)]
LN_SILU_DIMS = [8, 1024, 1032]


def head_rmsnorm_ref(x, w, heads, eps=EPS):
    """x bf16 [rows, >= heads 128]: gpu_util.rms_rope_ref on every head as a row of its own (float64
    statistics, the two roundings).  Returns (ref bf16 [rows, heads 128], bound)."""
    rows = x.shape[0]
    ref, bound = U.rms_rope_ref(x[:, :heads * HD].reshape(rows * heads, HD), w, eps)
    return ref.view(rows, heads * HD), bound.view(rows, heads * HD)


def ln_silu_ref(x, eps=EPS, norm=True):
    """out = bf16(silu(bf16(LN(x)))): LayerNorm without affine with float64 statistics, rounded to bf16, SiLU
    in float64, rounded to bf16.  bound: an fp32-level change of the statistics can flip bf16(n) by one ulp,
    at most 2^-7 |n|, which SiLU (slope within [-0.1, 1.1]) carries to at most 1.1 x that; plus one ulp,
    2^-7 |ref|, where the output rounding flips: ROW_BOUND (1.1 |n| + |ref|).  norm=False: SiLU alone."""
    n = U._ln_normalised(x, eps, torch.float64) if norm else x.double()
    nb = n.float().to(BF16)
    s64 = nb.double() * torch.sigmoid(nb.double())
    ref = s64.to(BF16)
    return ref, U.ROW_BOUND * (1.1 * n.abs() + ref.double().abs()), s64


def exact_pow2_rows(rows, dim, seed):
    """Rows of +-2^e (e in -2..2 per row, seeded signs): every head's mean square is 4^e exactly."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(-2, 3, (rows, 1), generator=g).float()
    sgn = torch.where(torch.rand((rows, dim), generator=g) < 0.5, -1.0, 1.0)
    return (sgn * torch.pow(2.0, e)).to(BF16)


# ------------------------------------------------------------------------------- vs_face_attn: geometry
def row_frames(batch, rpb, frames, tpf, tok_off):
    """(sample, frame, is_pad) of every row of a [batch * rpb, ...] call, by the header's rule."""
    r = torch.arange(batch * rpb)
    t = r % rpb + tok_off
    f = t // tpf
    return r // rpb, torch.clamp(f, max=frames - 1), f >= frames


def gather_kv(k, b, f, batch):
    """k [Bk, frames, N, H, 128] -> [rows, N, H, 128] for the rows' (sample, frame); Bk 1: one set for all."""
    return k[b if k.shape[0] == batch and batch > 1 else torch.zeros_like(b), f]


# ------------------------------------------------------------------------------ vs_face_attn: exact tier
EXACT_SCALE = 0.125
EXACT_A = 1024            # scale a = 128 >= 104: exp(-128) is below half the smallest fp32 denormal
EXACT_PATTERNS = {        # nkeys -> the score pattern t_j / a, rotated per (sample, frame)
    1: [(1,)],
    2: [(1, 1), (1, -1)],
    4: [(1, 1, 1, 1), (1, -1, 0, -1), (1, 1, -1, -1)],
    5: [(1, 1, -1, -1, 0)],
    8: [(1,) * 8, (1, 1, 1, 1, -1, -1, 0, 0), (1, -1, -1, -1, -1, 0, 0, 0), (1, 1, -1, -1, -1, -1, 0, 0)],
}
# (batch, rpb, heads, frames, tpf, nkeys, tok_off, pattern index, extra q columns): tokens_per_frame 1, 6, 63,
# 65; frames 1, 3; nkeys 1, 5, 8 (+ 2, 4 for the tie groups); heads 1, 2, 12, 40; a token_offset that crosses a
# frame inside the call; B = 2 with K / V per sample; ldq > heads 128; pad rows
EXACT_CASES = {
    "tpf1_f3_n5_h1": (1, 3, 1, 3, 1, 5, 0, 0, 0),
    "tpf6_f3_n5_h2_b2": (2, 18, 2, 3, 6, 5, 0, 0, 0),
    "tpf63_f3_n8_h12": (1, 189, 12, 3, 63, 8, 0, 1, 0),
    "tpf65_f3_n5_h40_b2_ld": (2, 195, 40, 3, 65, 5, 0, 0, 24),
    "tpf65_f1_n1_h2": (1, 65, 2, 1, 65, 1, 0, 0, 0),
    "offset_crosses_frame": (2, 70, 2, 3, 65, 5, 60, 0, 8),
    "pad_rows": (2, 40, 2, 3, 6, 5, 0, 0, 8),                    # 18 tokens, 22 pad rows per sample
    "offset_and_pad": (2, 12, 12, 3, 6, 8, 11, 3, 0),            # tokens 11..22: frames 1, 2 and 5 pad rows
    "ties_n2": (2, 130, 2, 1, 130, 2, 0, 1, 0),                  # more than one 128-token chunk per frame
    "ties_n2_all": (1, 18, 2, 3, 6, 2, 0, 0, 0),
    "ties_n4_single": (1, 18, 2, 3, 6, 4, 0, 1, 0),
    "ties_n4_all": (1, 18, 1, 3, 6, 4, 0, 0, 0),
    "ties_n8_all": (1, 18, 2, 3, 6, 8, 0, 0, 0),
    "ties_n8_single": (1, 18, 2, 3, 6, 8, 0, 2, 0),
}


def exact_problem(name):
    """Inputs on which every step of vs_face_attn but the final rounding is exact, and the answer by
    integer logic alone.

    u: a fixed +-1 pattern per head.  q = sigma 2^e u per (row, head) (e in -2..2, sigma = +-1 seeded): the
    head's mean square is 4^e, so bf16(q rsqrt(4^e + 1e-6)) = sigma u exactly.  wq in {1/2, 1, 2}: qn =
    sigma u wq.  Key j of (sample, frame, head) is t_j u[c] / (4 wq[c]) on four seeded columns c and zero
    elsewhere, t_j in {a, 0, -a}: every product qn k is sigma t_j / 4 and the score sigma t_j, an integer;
    times scale = 1/8 the gap between distinct scores is >= 128, so the softmax is 1 on the g keys that tie
    for the maximum and exactly 0 elsewhere (for either sigma), with g in {1, 2, 4, 8}: l = g, 1 / l exact.
    V holds integers -4..4 per (sample, frame, key, head, column): o = (sum over the tie group) / g, a
    multiple of 1/8 below 8 in magnitude -- a bf16 value, so the final rounding is exact too.
    Returns dict(q [rows, heads 128 + extra] with NaN sentinels outside the heads, k, v [B, frames, N, H, 128],
    wq [128], ref bf16 [rows, heads 128], pad [rows] bool, geometry)."""
    batch, rpb, heads, frames, tpf, nkeys, tok_off, pat, extra = EXACT_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    rows = batch * rpb
    u = torch.where(torch.rand((heads, HD), generator=g) < 0.5, -1.0, 1.0)
    sigma = torch.where(torch.rand((rows, heads, 1), generator=g) < 0.5, -1.0, 1.0)
    e = torch.randint(-2, 3, (rows, heads, 1), generator=g).float()
    q = sigma * torch.pow(2.0, e) * u
    wq = torch.pow(2.0, torch.randint(-1, 2, (HD,), generator=g).float())
    base = torch.tensor(EXACT_PATTERNS[nkeys][pat], dtype=torch.float32)
    t = torch.empty(batch, frames, nkeys)
    for b in range(batch):
        for f in range(frames):
            t[b, f] = torch.roll(base, shifts=f + 2 * b)
    k = torch.zeros(batch, frames, nkeys, heads, HD)
    cols = torch.stack([torch.randperm(HD, generator=g)[:4] for _ in range(batch * frames * nkeys * heads)])
    cols = cols.view(batch, frames, nkeys, heads, 4)
    val = (EXACT_A * t).view(batch, frames, nkeys, 1, 1) * u.expand(batch, frames, nkeys, heads, HD).gather(
        4, cols) / (4 * wq[cols])
    k.scatter_(4, cols, val)
    v = torch.randint(-4, 5, (batch, frames, nkeys, heads, HD), generator=g).float()
    b_, f_, pad = row_frames(batch, rpb, frames, tpf, tok_off)
    # integer logic: the tie group of sigma t
    st = sigma.view(rows, heads, 1) * t[b_, f_].view(rows, 1, nkeys)                 # [rows, H, N]
    tie = (st == st.max(dim=-1, keepdim=True).values).float()
    vv = v[b_, f_]                                                                   # [rows, N, H, 128]
    o = torch.einsum("rhn,rnhc->rhc", tie, vv) / tie.sum(-1, keepdim=True)
    o[pad] = 0
    qbuf = torch.full((rows, heads * HD + extra), float("nan"))
    qbuf[:, :heads * HD] = q.view(rows, heads * HD)
    return dict(q=qbuf.to(BF16), k=k.to(BF16), v=v.to(BF16), wq=wq.to(BF16), ref=o.view(rows, heads * HD).to(BF16),
                pad=pad, tie_sizes=sorted(set(tie.sum(-1).flatten().tolist())), last_key_in_tie=bool(tie[..., -1].any()),
                geom=dict(batch=batch, num_heads=heads, frames=frames, tokens_per_frame=tpf, nkeys=nkeys,
                          token_offset=tok_off), scale=EXACT_SCALE, exact=dict(k=k, v=v, o=o, q=q, wq=wq))


def exact_preconditions(p):
    """Every value of the exact problem is a bf16 value and the integer-logic answer equals the float64
    restatement of the contract."""
    ex = p["exact"]
    H = p["geom"]["num_heads"]
    for name in ("k", "v", "wq", "o"):
        assert torch.equal(ex[name].to(BF16).float(), ex[name]), name
    assert torch.equal(p["q"][:, :H * HD].float(), ex["q"].reshape(-1, H * HD))
    qn = head_rmsnorm_ref(p["q"], p["wq"], H)[0]
    assert torch.equal(qn.float().view(-1, H, HD), torch.sign(ex["q"]) * ex["wq"])           # sigma u wq, exactly
    o64, _, _ = face_attn_ref64(qn, p["k"], p["v"], scale=p["scale"], **p["geom"])
    assert torch.equal(o64.to(BF16).float(), p["ref"].float())                              # (-0 == +0)
    assert set(p["tie_sizes"]) <= {1.0, 2.0, 4.0, 8.0}


# ------------------------------------------------------------------------------ vs_face_attn: bound tier
BOUND_CASES = {"b2_tpf65_f3_n5_h12": (2, 195, 12, 3, 65, 5, 0), "b1_off_n8_h2": (1, 70, 2, 3, 65, 8, 60),
               "b2_n1_h1": (2, 18, 1, 3, 6, 1, 0)}
FA_WINDOW = 2.0 ** -20      # x A: the kernel-order fp32 restatement against the device (see face_attn_order32)
FA_MAX_AMBIGUOUS = 0.01


def bound_inputs(name):
    """q ~ 2 N(0, 1) with, per sample, one all-zero (row, head) and one at 2^-12 N(0, 1) (there the norm's eps
    decides the result); k, v ~ N(0, 1); wq = 1 + 0.1 N."""
    batch, rpb, heads, frames, tpf, nkeys, tok_off = BOUND_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    q = 2.0 * torch.randn((batch * rpb, heads, HD), generator=g)
    for b in range(batch):
        q[b * rpb + 1, 0] = 0
        q[b * rpb + min(3, rpb - 1), heads - 1] *= 2.0 ** -13
    k = torch.randn((batch, frames, nkeys, heads, HD), generator=g)
    v = torch.randn((batch, frames, nkeys, heads, HD), generator=g)
    wq = 1 + 0.1 * torch.randn(HD, generator=g)
    return dict(q=q.view(-1, heads * HD).to(BF16), k=k.to(BF16), v=v.to(BF16), wq=wq.to(BF16), scale=HD ** -0.5,
                geom=dict(batch=batch, num_heads=heads, frames=frames, tokens_per_frame=tpf, nkeys=nkeys,
                          token_offset=tok_off))


def face_attn_ref64(qn, k, v, *, batch, num_heads, frames, tokens_per_frame, nkeys, token_offset, scale):
    """The contract in float64 over an already normalised qn (bf16 [rows, >= H 128]): returns (o [rows, H 128],
    A = sum_j p_j |v_j| / l, smag = scale max_j sum_c |qn_c k_jc| per (row, head) [rows, H, 1]); pad rows 0."""
    rows, H = qn.shape[0], num_heads
    b, f, pad = row_frames(batch, rows // batch, frames, tokens_per_frame, token_offset)
    kk = gather_kv(k, b, f, batch).double()                                          # [rows, N, H, 128]
    vv = gather_kv(v, b, f, batch).double()
    q = qn[:, :H * HD].double().view(rows, 1, H, HD)
    s = scale * (q * kk).sum(-1)                                                     # [rows, N, H]
    p = torch.softmax(s, dim=1)
    o = (p.unsqueeze(-1) * vv).sum(1)
    A = (p.unsqueeze(-1) * vv.abs()).sum(1)
    smag = scale * (q.abs() * kk.abs()).sum(-1).max(dim=1).values
    o[pad], A[pad] = 0, 0
    return o.view(rows, H * HD), A.view(rows, H * HD), smag.view(rows, H, 1)


def face_attn_within(got, o, A, smag, nkeys):
    """|got - o| <= half_ulp(|o| + slack A) + slack A per element, from the rounding points alone:
      * a score is a 128-term fp32 dot product (any summation order: at most 128 u sum |qn k|, u = 2^-24),
        one product with scale and one subtraction of the maximum: |d(s_j - m)| <= 2 * 131 u smag =: E
        (both s_j and m move);
      * expf within 2 ulp: p_j (1 + 4 u); so every weight p_j / l moves by a factor within exp(+-2 (E + 4 u)),
        and |o' - o| <= expm1(2 (E + 4 u)) sum_j w_j |v_j| = expm1(..) A;
      * the fp32 sums over the nkeys terms of p v and of l, the reciprocal and the product: (2 nkeys + 4) u A;
      * the output rounding: half a bf16 ulp of the value o' that is rounded, |o'| <= |o| + slack A.  bf16
        keeps 8 significant bits, so half an ulp of x is 2^(floor(log2 |x|) - 8): between 2^-9 |x| (x just
        below a power of two) and 2^-8 |x| (x at one).  A flat 2^-9 |o| is below that for most values -- o =
        2.0052 lies between the bf16 neighbours 2 and 2.015625 and its correct rounding is 0.0052 away, more
        than 2^-9 |o| = 0.0039 -- so the term is the half ulp itself, the tightest bound a correct rounding
        meets.
    The reference reads the device's own qn (vs_head_rmsnorm, bit-identical to the fused norm), so the norm
    adds nothing."""
    u = 2.0 ** -24
    E = 2 * 131 * u * smag
    slack = torch.expm1(2 * (E + 4 * u)) + (2 * nkeys + 4) * u                      # [rows, H, 1]
    rows, H = smag.shape[0], smag.shape[1]
    sA = (slack * A.view(rows, H, HD)).view(rows, H * HD)
    top = o.abs() + sA
    half_ulp = torch.pow(torch.tensor(2.0, dtype=torch.float64),
                         torch.floor(torch.log2(torch.clamp(top, min=2.0 ** -126))) - 8)
    bound = torch.where(top > 0, half_ulp, torch.zeros_like(top)) + sA
    d = (got.double() - o).abs()
    return d <= bound, (d - bound).max().item()


def _fma32(a, b, c):
    """fl32(a b + c): the product of two fp32 values is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


def _row16(x):
    """The DPP tree of csrc/animate.hip over the last axis of 16 lanes: pairs, quads, halves, the row."""
    for _ in range(4):
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def head_rmsnorm_order32(x, w, heads, eps=EPS, drop_eps=False, apply_w=True):
    """vs_head_rmsnorm in fp32 in the kernel's order: each lane's 8 squares by fused multiply-add in column
    order, the 16 partial sums by the DPP tree, rsqrt(s / 128 + eps), the two roundings."""
    rows = x.shape[0]
    xf = x[:, :heads * HD].float().view(rows, heads, 16, 8)
    s = torch.zeros(rows, heads, 16)
    for e in range(8):
        s = _fma32(xf[..., e], xf[..., e], s)
    r = torch.rsqrt(_row16(s) * (1.0 / 128.0) + (0.0 if drop_eps else torch.tensor(eps, dtype=torch.float32)))
    n = (xf * r.view(rows, heads, 1, 1)).to(BF16).float()
    if apply_w:
        n = (n * w.float().view(1, 1, 16, 8)).to(BF16).float()
    return n.view(rows, heads * HD).to(BF16)


def face_attn_order32(qn, k, v, *, batch, num_heads, frames, tokens_per_frame, nkeys, token_offset, scale,
                      drop_last_key=False, frame_shift=0, swap_samples=False):
    """vs_face_attn after the norm in fp32 in the kernel's order (the float32 restatement): per lane the 8
    products of a score by fused multiply-add in column order, the DPP tree, one product with scale; p =
    exp(s - m); l and the 8 accumulators over the keys in key order (fused multiply-add); acc * (1 / l); one
    rounding.  Against the device only expf (2 ulp), the reciprocal and the products can differ, each by an
    ulp or two of p, l or o: a few fp32 ulp of A = sum p |v| / l.  FA_WINDOW = 2^-20 A (16 ulp) is that with
    a factor of two; an element whose float64 value is within it of a bf16 rounding midpoint is ambiguous.
    The keyword mutations are the WRONG variants of tests/test_animate_cpu.py."""
    rows, H = qn.shape[0], num_heads
    rpb = rows // batch
    b, f, pad = row_frames(batch, rpb, frames, tokens_per_frame, token_offset)
    if frame_shift:         # the frame index of a frame's first token taken from the frame before
        t = torch.arange(rows) % rpb + token_offset
        f = torch.where((t % tokens_per_frame == 0) & (f > 0), f - 1, f)
    if swap_samples:
        b = (batch - 1) - b
    n = nkeys - 1 if drop_last_key else nkeys
    if n == 0:              # (no key left: 0 / 0)
        return torch.full((rows, H * HD), float("nan")).to(BF16)
    kk = gather_kv(k, b, f, batch).float().view(rows, nkeys, H, 16, 8)
    vv = gather_kv(v, b, f, batch).float().view(rows, nkeys, H, HD)
    q = qn[:, :H * HD].float().view(rows, H, 16, 8)
    s = []
    for j in range(n):
        d = torch.zeros(rows, H, 16)
        for e in range(8):
            d = _fma32(q[..., e], kk[:, j, ..., e], d)
        s.append(torch.tensor(scale, dtype=torch.float32) * _row16(d))
    s = torch.stack(s, dim=-1)                                                       # [rows, H, n]
    m = s.max(dim=-1, keepdim=True).values
    p = torch.exp(s - m)
    l = torch.zeros(rows, H)
    acc = torch.zeros(rows, H, HD)
    for j in range(n):
        l = l + p[..., j]
        acc = _fma32(p[..., j].unsqueeze(-1), vv[:, j], acc)
    o = acc * (1.0 / l).unsqueeze(-1)
    o[pad] = 0
    return o.view(rows, H * HD).to(BF16)


def near_midpoint_abs(x64, tol):
    """True where the float64 value is within `tol` (absolute, per element) of a bf16 rounding midpoint."""
    a = x64.abs()
    e = torch.floor(torch.log2(torch.clamp(a, min=2.0 ** -126)))
    ulp = torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)                  # the bf16 spacing at a
    r = torch.remainder(a / ulp, 1.0)
    return ((r - 0.5).abs() * ulp <= tol) & (a > 0)


def face_attn_ambiguous(o64, A):
    return near_midpoint_abs(o64, FA_WINDOW * A)


def emulate(p, **mut):
    """The fp32 CPU emulation of the whole contract on a problem dict (exact or bound inputs); norm mutations
    drop_eps / no_wq, attention mutations as face_attn_order32."""
    H = p["geom"]["num_heads"]
    qn = head_rmsnorm_order32(p["q"], p["wq"], H, drop_eps=mut.pop("drop_eps", False), apply_w=not mut.pop("no_wq", False))
    return face_attn_order32(qn, p["k"], p["v"], scale=p["scale"], **p["geom"], **mut)


MUTATIONS = {"eps dropped": dict(drop_eps=True), "wq not applied": dict(no_wq=True),
             "last key dropped": dict(drop_last_key=True), "frame index off by one at a frame edge": dict(frame_shift=1),
             "K/V of the wrong CFG sample": dict(swap_samples=True)}


def bf16_all_finite():
    """Every finite bf16 bit pattern + 37 seeded extras (gpu_util.t5_gelu_inputs' set)."""
    _, g = U.t5_gelu_inputs()
    return g[torch.isfinite(g.float())]


def silu64(x):
    x64 = x.double()
    return x64 / (1.0 + torch.exp(-x64))
