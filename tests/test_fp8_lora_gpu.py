"""The hot-loaded (un-merged) LoRA on fp8 layers: vs_gemm_fp8_lora, the bf16 second K phase of
gemm_fp8_tn_8p (csrc/gemm.hip), through kernels.gemm_fp8(a2=, w2=), models.linear and
hotload_lora(fp8_layers="fuse").

Reference: AutoWrappedLinear.forward (diffsynth/vram_management/layers.py:168-182): out =
fp8_linear(x, W, b) (:115-151), then out + x A^T B^T in bf16.  The kernel computes
bf16(s[m] * (x8 . W8^T) + t . B^T + b) with t = bf16(x (alpha A)^T): one fp32 sum, one rounding.

Integer-valued operands keep every partial sum exact, so the kernel must equal that formula bit for
bit (whatever its summation order): the MFMA operand maps of both phases, the phase switch in either
LDS buffer, the row scale on the fp8 product only, both epilogue widths.  Random data: within the
tolerance the bf16 hot-load path's tests use, against the reference's own rounding points."""
import pytest
import torch
import torch.nn as nn

from gpu_util import BF16, err
from oracle import wan_oracle as O

pytestmark = pytest.mark.gpu
E4M3 = torch.float8_e4m3fn


def _k():
    from vstyler import kernels as K
    return K


def _quant(K, x):
    x8 = torch.empty(x.shape, dtype=torch.uint8, device="cuda")
    sc = torch.empty(x.shape[0], dtype=torch.float32, device="cuda")
    K.quant_fp8_rows(x.cuda(), x8, sc)
    return x8, sc


def _integer_case(M, N, Kd, k2, seed):
    """Operands of an exact case (CPU): x integer-valued with every third row scaled by exactly 2
    (one element 896 = 2 * 448, the rest even integers in [-8, 8]: s = 2.0, s + 1e-8 == 2.0f, the
    halved row exact in e4m3; every other row max <= 448: s = 1), w in [-3, 3] with an asymmetric
    first column, t / B in [-2, 2], integer bias."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (M, Kd), generator=g)
    x[::3] *= 2
    x[::3, 5] = 896
    w = torch.randint(-3, 4, (N, Kd), generator=g)
    w[:, 0] += torch.arange(N) % 7
    t = torch.randint(-2, 3, (M, k2), generator=g)
    lb = torch.randint(-2, 3, (N, k2), generator=g)
    b = torch.randint(-8, 9, (N,), generator=g)
    return tuple(v.to(BF16) for v in (x, w, t, lb, b))


def _exact_y(x8, sc, w, t, lb, b):
    """bf16(s[m] * (x8f @ w^T) + t @ B^T + b) on the CPU from the bytes / scales the kernel read,
    after checking that the fp32 and fp64 evaluations of the sum agree (every partial sum exact:
    the bit-for-bit comparison is legitimate)."""
    x8f = x8.cpu().view(E4M3)
    s = sc.cpu()
    assert set(s.tolist()) == {1.0, 2.0} and torch.equal(s[::3], torch.full_like(s[::3], 2.0))

    def total(dt):
        return s.to(dt)[:, None] * (x8f.to(dt) @ w.to(dt).t()) + t.to(dt) @ lb.to(dt).t() + b.to(dt)
    y32, y64 = total(torch.float32), total(torch.float64)
    assert torch.equal(y32.double(), y64)
    return y32.to(BF16)


@pytest.mark.parametrize("M,N,Kd,k2", [(300, 260, 128, 64),      # one fp8 K-tile + one LoRA tile, ragged M, 8-B epilogue
                                       (520, 384, 384, 128),     # odd fp8 tile count: the switch lands on buffer 1
                                       (513, 520, 256, 192),     # even count; two stacked adapters' worth of rank
                                       (256, 256, 640, 64)])     # a full, aligned tile
def test_gemm_fp8_lora_integer_exact(M, N, Kd, k2):
    K = _k()
    x, w, t, lb, b = _integer_case(M, N, Kd, k2, seed=M + N + Kd + k2)
    x8, sc = _quant(K, x)
    out = torch.full((M, N), 7.0, dtype=BF16, device="cuda")
    K.gemm_fp8(x8, sc, w.to(E4M3).view(torch.uint8).cuda(), out, bias=b.cuda(), a2=t.cuda(), w2=lb.cuda())
    torch.cuda.synchronize()
    ref = _exact_y(x8, sc, w, t, lb, b)
    o = out.cpu()
    bad = (o != ref)
    print(f"fp8+LoRA exact {M}x{N}x{Kd}+{k2}: {int(bad.sum())} mismatches"
          f"{'' if not bad.any() else ' first at ' + str(bad.nonzero()[0].tolist())}")
    assert torch.equal(o, ref)


def test_gemm_fp8_lora_epilogues_exact():
    """GELU, gate-residual + hint and residual-with-alpha on top of the exact y, the output aliasing
    the residual as the model uses it (two gate batches)."""
    K = _k()
    M, N, Kd, k2, S = 600, 520, 384, 128, 300
    x, w, t, lb, b = _integer_case(M, N, Kd, k2, seed=17)
    x8, sc = _quant(K, x)
    y = _exact_y(x8, sc, w, t, lb, b)
    w8 = w.to(E4M3).view(torch.uint8).cuda()
    kw = dict(bias=b.cuda(), a2=t.cuda(), w2=lb.cuda())
    res = torch.randn(M, N, generator=torch.Generator().manual_seed(4)).to(BF16)
    gate = (0.25 * torch.randn(2, N, generator=torch.Generator().manual_seed(5))).to(BF16)
    hint = torch.randn(M, N, generator=torch.Generator().manual_seed(6)).to(BF16)
    out = torch.empty(M, N, dtype=BF16, device="cuda")
    K.gemm_fp8(x8, sc, w8, out, epilogue=K.VS_EPI_GELU, **kw)
    # GELU: the kernel's sigma form vs torch's tanh form differ by <= 1 ulp on the cancellation zone
    ref = O.gelu_tanh(y)
    d = (out.cpu().float() - ref.float()).abs()
    assert (d <= ref.float().abs() * 2 ** -7 + 1e-6).all()
    xo = res.cuda()
    K.gemm_fp8(x8, sc, w8, xo, epilogue=K.VS_EPI_GATE_RES, residual=xo, gate=gate.cuda(), gate_bstride=N,
               rows_per_batch=S, hint=hint.cuda(), hint_scale=0.5, **kw)
    ref = torch.cat([O.gate_residual(res[:S], gate[0], y[:S]), O.gate_residual(res[S:], gate[1], y[S:])])
    ref = O.add(ref, O.bf(hint.float() * 0.5))
    assert torch.equal(xo.cpu(), ref)
    xo = res.cuda()
    K.gemm_fp8(x8, sc, w8, xo, epilogue=K.VS_EPI_RES, residual=xo, alpha=0.125, **kw)
    assert torch.equal(xo.cpu(), O.add(res, O.bf(0.125 * y.float())))


def test_gemm_fp8_lora_empty_phase_is_vs_gemm_fp8():
    """k2 == 0 through the new entry point: vs_gemm_fp8 bit for bit."""
    K = _k()
    M, N, Kd = 700, 520, 640
    g = torch.Generator(device="cuda").manual_seed(23)
    x = torch.randn(M, Kd, device="cuda", generator=g).to(BF16)
    x[::4] *= 900.0
    w8 = (0.05 * torch.randn(N, Kd, device="cuda", generator=g)).to(E4M3).view(torch.uint8)
    b = (0.1 * torch.randn(N, device="cuda", generator=g)).to(BF16)
    x8, sc = _quant(K, x)
    plain = torch.empty(M, N, dtype=BF16, device="cuda")
    K.gemm_fp8(x8, sc, w8, plain, bias=b)
    empty = torch.full((M, N), 7.0, dtype=BF16, device="cuda")
    K.gemm_fp8(x8, sc, w8, empty, bias=b, a2=torch.empty(M, 0, dtype=BF16, device="cuda"),
               w2=torch.empty(N, 0, dtype=BF16, device="cuda"))
    assert torch.equal(plain, empty)


def _fp8_linear_module(D, w, b):
    from vstyler.models import Linear
    m = nn.Module()
    m.add_module("q", Linear(D, D, device="cuda"))
    m.q.weight.data.copy_(w)
    m.q.bias.data.copy_(b)
    m.q.weight_fp8 = m.q.weight.detach().to(E4M3).view(torch.uint8).contiguous()      # as quantize_fp8_
    return m


def _ref_fp8_lora(x, w, b, adapters):
    """The reference's rounding points (layers.py:168-185): fp8_linear, then one bf16 add of
    bf16(bf16(x (alpha A)^T) B^T) per adapter."""
    ref = O.fp8_linear(x, w, b)
    for a_s, up in adapters:
        t = O.bf(x.float() @ a_s.float().t())
        ref = O.bf(ref.float() + O.bf(t.float() @ up.float().t()).float())
    return ref


def test_linear_fp8_hotload_random():
    from vstyler.lora import hotload_lora
    from vstyler.models import Workspace, linear
    g = torch.Generator().manual_seed(90)
    D, r = 256, 32
    w = (0.05 * torch.randn(D, D, generator=g)).to(BF16)
    b = (0.01 * torch.randn(D, generator=g)).to(BF16)
    up = (0.05 * torch.randn(D, r, generator=g)).to(BF16)
    down = (0.05 * torch.randn(r, D, generator=g)).to(BF16)
    x = torch.randn(100, D, generator=g).to(BF16)
    m = _fp8_linear_module(D, w, b)
    ws = Workspace("cuda")
    base = torch.empty(100, D, dtype=BF16, device="cuda")
    linear(m.q, x.cuda(), base, ws)
    assert err(base, O.fp8_linear(x, w, b))[1] < 1e-2
    assert hotload_lora(m, {"q.lora_A.default.weight": down, "q.lora_B.default.weight": up}, alpha=0.7,
                        fp8_layers="fuse") == 1
    out = torch.empty(100, D, dtype=BF16, device="cuda")
    linear(m.q, x.cuda(), out, ws)
    ref = _ref_fp8_lora(x, w, b, [(O.bf(down.float() * 0.7), up)])
    rl, moved = err(out, ref)[1], err(out, base)[1]
    print(f"fp8 + hot-loaded LoRA linear: rel-L2 {rl:.4g} vs the reference, {moved:.4g} away from the bare fp8 output")
    assert rl < 1e-2
    assert moved > 1e-2                          # the term cannot silently drop


def test_linear_fp8_two_hotloaded_loras_add_up():
    from vstyler.lora import hotload_lora
    from vstyler.models import Workspace, linear
    g = torch.Generator().manual_seed(92)
    D = 256
    w = (0.05 * torch.randn(D, D, generator=g)).to(BF16)
    b = (0.01 * torch.randn(D, generator=g)).to(BF16)
    m = _fp8_linear_module(D, w, b)
    adapters = []
    for r, alpha in ((32, 0.7), (96, 1.3)):
        up = (0.05 * torch.randn(D, r, generator=g)).to(BF16)
        down = (0.05 * torch.randn(r, D, generator=g)).to(BF16)
        assert hotload_lora(m, {"q.lora_A.default.weight": down, "q.lora_B.default.weight": up}, alpha=alpha,
                            fp8_layers="fuse") == 1
        adapters.append((O.bf(down.float() * alpha), up))
    assert m.q.lora_A.shape == (64 + 128, D) and m.q.lora_B.shape == (D, 64 + 128)
    x = torch.randn(100, D, generator=g).to(BF16)
    out = torch.empty(100, D, dtype=BF16, device="cuda")
    linear(m.q, x.cuda(), out, Workspace("cuda"))
    ref = _ref_fp8_lora(x, w, b, adapters)
    one = _ref_fp8_lora(x, w, b, adapters[:1])
    assert err(one, ref)[1] > 1e-2               # the second adapter is not negligible
    assert err(out, ref)[1] < 1e-2


TARGETS = [f"{a}.{l}" for a in ("self_attn", "cross_attn") for l in "qkvo"] + ["ffn.0", "ffn.2"]


def _tiny_fp8_with_lora(seed=5, alpha=2.0):
    """The tiny DiT+VACE with fp8 block linears and a rank-32 LoRA for the VACE blocks' ten linears
    (state dict in the reference's peft layout); returns the models before the hot-load.  alpha 2
    puts the adapter's effect on the output well above the acceptance bound of the forward test, so
    a forward that dropped the adapter could not pass it."""
    from test_model_gpu import build
    from vstyler.models import quantize_fp8_
    cfg = O.WAN_CONFIGS["tiny"]
    W = O.random_weights(cfg, seed=seed)
    dit, vace = build(cfg, W)
    quantize_fp8_(dit)
    quantize_fp8_(vace)
    g = torch.Generator().manual_seed(8)
    r, D, F = 32, cfg["dim"], cfg["ffn_dim"]
    lora = {}
    for i in range(len(cfg["vace_layers"])):
        for t in TARGETS:
            out_f, in_f = {"ffn.0": (F, D), "ffn.2": (D, F)}.get(t, (D, D))
            lora[f"vace_blocks.{i}.{t}.lora_A.default.weight"] = (0.05 * torch.randn(r, in_f, generator=g)).to(BF16)
            lora[f"vace_blocks.{i}.{t}.lora_B.default.weight"] = (0.05 * torch.randn(out_f, r, generator=g)).to(BF16)
    return cfg, W, dit, vace, lora, alpha


def test_model_fn_fp8_hotload_tiny_vs_oracle(monkeypatch):
    """Config 5 with a hot-loaded VACE LoRA against the oracle with FP8_BLOCK_LINEARS and HOTLOAD,
    its lora_linear taking fp8_linear for the base term (layers.py:168-182); acceptance: the fp8
    tiny forward's floor rule (the oracle's own fp32-vs-fp64 distance)."""
    from vstyler import model_fn_wan_video
    from vstyler.lora import hotload_lora
    cfg, W, dit, vace, lora, alpha = _tiny_fp8_with_lora()
    lat, cp, cn, vc = O.synthetic_inputs(cfg, 5, 128, 128)
    t = torch.tensor([900.0]).to(BF16)
    run = lambda: model_fn_wan_video(dit, vace=vace, latents=lat.cuda(), timestep=t.cuda(), context=cp.cuda(),
                                     vace_context=vc.cuda()).clone()
    bare = run()
    assert hotload_lora(vace, lora, alpha, fp8_layers="fuse") == len(TARGETS) * len(cfg["vace_layers"])
    out = run()

    def lora_linear_fp8(x, w, b, lora_a, lora_b):
        y = O.fp8_linear(x, w, b)
        tt = O.bf(x.float() @ lora_a.float().t())
        return O.bf(y.float() + O.bf(tt.float() @ lora_b.float().t()).float())
    monkeypatch.setattr(O, "lora_linear", lora_linear_fp8)
    monkeypatch.setattr(O, "FP8_BLOCK_LINEARS", True)
    for i in range(len(cfg["vace_layers"])):
        for tg in TARGETS:
            la, lb = (lora[f"vace_blocks.{i}.{tg}.lora_{x}.default.weight"] for x in "AB")
            monkeypatch.setitem(O.HOTLOAD, id(W[f"vace_blocks.{i}.{tg}.weight"]), (O.bf(la.float() * alpha), lb))
    ref = O.model_fn(W, cfg, lat, t, cp, vc)
    monkeypatch.setattr(O, "ACC_DTYPE", torch.float64)
    ref64 = O.model_fn(W, cfg, lat, t, cp, vc)
    fmx, frl = err(ref64, ref)
    mx, rl = err(out, ref)
    dmx, drl = err(out, bare)
    print(f"fp8 + hot-load tiny forward: max-abs {mx:.4g} rel-L2 {rl:.4g} (floor {fmx:.4g} / {frl:.4g}); "
          f"{dmx:.4g} / {drl:.4g} away from the forward without the adapter")
    assert rl <= 1.5 * frl + 2e-3 and mx <= 1.5 * fmx + 2e-2
    assert drl > 1.5 * frl + 2e-3 and dmx > 1.5 * fmx + 2e-2       # the adapter's effect is above the floor


def test_denoise_fp8_hotload_graph_replay_bit_identical_to_eager():
    """The captured step (WanVideoPipeline.denoise(use_graph=True), as test_model_gpu's stepper test)
    with fp8 block linears and the hot-loaded LoRA replays to exactly the eager loop's latents."""
    from vstyler import WanVideoPipeline
    from vstyler.lora import hotload_lora
    cfg, W, dit, vace, lora, alpha = _tiny_fp8_with_lora()
    hotload_lora(vace, lora, alpha, fp8_layers="fuse")
    pipe = WanVideoPipeline(device="cuda")
    pipe.dit, pipe.vace = dit, vace
    lat, cp, cn, vc = O.synthetic_inputs(cfg, 5, 128, 128)
    eager = pipe.denoise(lat, cp.cuda(), cn.cuda(), vc.cuda(), num_inference_steps=4, use_graph=False)
    assert pipe.last_graph is None
    graph = pipe.denoise(lat, cp.cuda(), cn.cuda(), vc.cuda(), num_inference_steps=4, use_graph=True)
    assert pipe.last_graph is not None
    assert torch.equal(eager, graph)
