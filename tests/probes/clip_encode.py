"""Cost of WanImageEncoder.encode_image at the real dims (ViT-H/14: 1280 / 16 heads of 80 / 5120, 32 layers
of which 31 run, 257 tokens), random weights, one image and two images, and what the zero-padded head
layout (heads of 80 in 128 columns for vs_attn_fwd) costs inside it.

(a) encode_image end to end: HIP events around back-to-back calls (at least ITERS, and enough for a window of 1.5 s), WINDOWS windows per batch size,
    the two batch sizes alternating; median and spread (max - min) between windows.
(b) the three padded launches of one block at the same row counts, the 31 blocks' worth per call:
      qkv_padded   to_qkv GEMM, N = 3 * 16 * 128          qkv_compact   the same GEMM at N = 3 * 1280
      proj_padded  proj GEMM, K = 16 * 128                 proj_compact  the same GEMM at K = 1280
      attn_padded  vs_attn_fwd over the padded heads
    The compact GEMMs are what a native width-80 attention kernel would leave; of attn_padded such a kernel
    could save at most the padded share of its arithmetic (48 / 128).

  python tests/probes/clip_encode.py [--iters 20] [--windows 5] [--out FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "video-styler_amd"))
import torch

from vstyler import kernels as K
from vstyler.clip import WanImageEncoder, attention_d80

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--out", default=None, help="also write the log lines to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
BF16 = torch.bfloat16
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def events(fn, iters):
    """ms per call: HIP events around `iters` back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def summary(ms):
    v = sorted(ms)
    return f"median {v[len(v) // 2]:.3f} ms, spread {v[-1] - v[0]:.3f} ms, windows {[round(x, 3) for x in ms]}"


enc = WanImageEncoder(device=dev).init_random_(seed=8)
g = torch.Generator(device=dev).manual_seed(3)
frames = {n: (2 * torch.rand((n, 3, 480, 832), generator=g, device=dev) - 1).to(BF16) for n in (1, 2)}
say(f"encode_image, ViT-H/14, {enc.num_layers - 1} blocks, 480x832 frames, {args.iters} calls per window, "
    f"{args.windows} windows per batch size (alternating)")
iters = {}
for n in (1, 2):
    events(lambda: enc.encode_image(frames[n]), 3)                 # warm every shape
    once = events(lambda: enc.encode_image(frames[n]), 5)
    iters[n] = max(args.iters, int(1500.0 / once) + 1)             # a window well over a second
ms = {1: [], 2: []}
for _ in range(args.windows):
    for n in (1, 2):
        ms[n].append(events(lambda: enc.encode_image(frames[n]), iters[n]))
for n in (1, 2):
    say(f"  n = {n}: {summary(ms[n])} ({iters[n]} calls, window "
        f"{iters[n] * sorted(ms[n])[len(ms[n]) // 2] / 1000:.2f} s)")

D, H, T, L = enc.dim, enc.num_heads, enc.tokens, enc.num_layers - 1
for n in (1, 2):
    M = n * T

    def rnd(*shape):
        return torch.randn(shape, generator=g, device=dev).to(BF16)
    h, o_pad, o_cmp = rnd(M, D), rnd(M, H * 128), rnd(M, D)
    w_qkv_pad, w_qkv_cmp = enc.w["0.attn.to_qkv.weight"], rnd(3 * D, D) / 36
    b_pad, b_cmp = enc.w["0.attn.to_qkv.bias"], rnd(3 * D)
    w_proj_pad, w_proj_cmp = enc.w["0.attn.proj.weight"], rnd(D, D) / 36
    qkv_pad, qkv_cmp = torch.empty(M, 3 * H * 128, dtype=BF16, device=dev), torch.empty(M, 3 * D, dtype=BF16, device=dev)
    x, att = rnd(M, D), torch.empty(M, H * 128, dtype=BF16, device=dev)
    K.gemm(h, w_qkv_pad, qkv_pad, bias=b_pad)
    sections = {
        "qkv_padded": lambda: K.gemm(h, w_qkv_pad, qkv_pad, bias=b_pad),
        "qkv_compact": lambda: K.gemm(h, w_qkv_cmp, qkv_cmp, bias=b_cmp),
        "proj_padded": lambda: K.gemm(o_pad, w_proj_pad, x, epilogue=K.VS_EPI_RES, residual=x),
        "proj_compact": lambda: K.gemm(o_cmp, w_proj_cmp, x, epilogue=K.VS_EPI_RES, residual=x),
        "attn_padded": lambda: attention_d80(qkv_pad, att, H, n),
    }
    for fn in sections.values():
        events(fn, 3)
    sec = {k: [] for k in sections}
    for _ in range(args.windows):
        for name, fn in sections.items():
            sec[name].append(L * events(fn, 10 * args.iters))
    say(f"sections at n = {n}, ms per encode_image ({L} blocks' worth), {args.windows} windows alternating:")
    for name in sections:
        say(f"  {name}: {summary(sec[name])}")
    med = {k: sorted(v)[len(v) // 2] for k, v in sec.items()}
    gemm_gain = med["qkv_padded"] - med["qkv_compact"] + med["proj_padded"] - med["proj_compact"]
    attn_gain = med["attn_padded"] * 48 / 128
    total = sorted(ms[n])[len(ms[n]) // 2]
    say(f"  the padding's cost at n = {n}: GEMMs {gemm_gain:.3f} ms measured, attention at most {attn_gain:.3f} ms "
        f"(48/128 of attn_padded) of {total:.3f} ms per call: {100 * (gemm_gain + attn_gain) / total:.1f} % at most")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
