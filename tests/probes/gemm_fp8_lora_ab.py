"""A/B: the fp8 GEMM with the un-merged LoRA fused as its bf16 second K phase (vs_gemm_fp8_lora)
against its yardsticks, per 14B VACE-block GEMM with the epilogue that layer uses, rank 128:
  a   fp8 + LoRA, one launch (gemm_fp8_tn_8p<LORA>)
  b   plain vs_gemm_fp8, no LoRA (the default 4-wave kernel; b8: the 8-phase kernel a is built on)
  c   the bf16 hot-load vs_gemm(..., a2, w2) (gemm_bf16_tn_8p<LORA>)
  d   bias epilogue only: vs_gemm_fp8, then vs_gemm(t, B, C, VS_EPI_RES, residual=C) (two launches)
The LoRA down-projection t = x (alpha A)^T is the same extra launch for a, c and d and is not timed.
Interleaved rounds in one process after a warm-up of every form; each sample is REPS back-to-back
launches between device events; min and median over the rounds.
usage: gemm_fp8_lora_ab.py [--out FILE] [--rounds N] [M ...]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "video-styler_amd"))
import torch
from vstyler import kernels as K

BF16 = torch.bfloat16
REPS = 5
RANK = 128


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


SHAPES = (("qkv-like bias", 5120, 5120, K.VS_EPI_BIAS), ("o-proj gate-res", 5120, 5120, K.VS_EPI_GATE_RES),
          ("ffn-up gelu", 13824, 5120, K.VS_EPI_GELU), ("ffn-down gate-res", 5120, 13824, K.VS_EPI_GATE_RES))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("rows", nargs="*", type=int)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"fp8 + LoRA A/B: rank {RANK}, {REPS} launches per sample, {args.rounds} interleaved rounds; ms = min (median)")
    for M in args.rows or (59280,):
        for name, N, Kd, epi in SHAPES:
            g = torch.Generator(device="cuda").manual_seed(1)
            a = torch.randn(M, Kd, device="cuda", generator=g).to(BF16)
            w = (0.05 * torch.randn(N, Kd, device="cuda", generator=g)).to(BF16)
            w8 = w.to(torch.float8_e4m3fn).view(torch.uint8)
            a8 = torch.empty(M, Kd, dtype=torch.uint8, device="cuda")
            sc = torch.empty(M, dtype=torch.float32, device="cuda")
            K.quant_fp8_rows(a, a8, sc)
            la = (0.02 * torch.randn(RANK, Kd, device="cuda", generator=g)).to(BF16)
            lb = (0.02 * torch.randn(N, RANK, device="cuda", generator=g)).to(BF16)
            t = torch.empty(M, RANK, dtype=BF16, device="cuda")
            K.gemm(a, la, t)
            b = (0.1 * torch.randn(N, device="cuda", generator=g)).to(BF16)
            gate = (0.1 * torch.randn(2, N, device="cuda", generator=g)).to(BF16)
            out = torch.randn(M, N, device="cuda", generator=g).to(BF16)
            kw = dict(epilogue=epi, bias=b)
            if epi == K.VS_EPI_GATE_RES:
                kw.update(residual=out, gate=gate, gate_bstride=N, rows_per_batch=(M + 1) // 2)

            def two_launches():
                K.gemm_fp8(a8, sc, w8, out, bias=b)
                K.gemm(t, lb, out, epilogue=K.VS_EPI_RES, residual=out)

            def plain8():
                with K.options(gemm_kernel=8):
                    K.gemm_fp8(a8, sc, w8, out, **kw)
            forms = {"a": lambda: K.gemm_fp8(a8, sc, w8, out, a2=t, w2=lb, **kw),
                     "b": lambda: K.gemm_fp8(a8, sc, w8, out, **kw),
                     "b8": plain8,
                     "c": lambda: K.gemm(a, w, out, a2=t, w2=lb, **kw)}
            if epi == K.VS_EPI_BIAS:
                forms["d"] = two_launches
            for fn in forms.values():               # warm-up: code objects, workspaces
                fn()
                fn()
            torch.cuda.synchronize()
            ts = {v: [] for v in forms}
            for _ in range(args.rounds):
                for v, fn in forms.items():
                    ts[v].append(timed(fn))
            fl = {v: 2.0 * M * N * (Kd + (0 if v in ("b", "b8") else RANK)) for v in forms}
            best = {v: min(x) for v, x in ts.items()}
            say(f"M={M} {name:18s} N={N} K={Kd}: " +
                "  ".join(f"{v} {best[v]:.3f} ({statistics.median(ts[v]):.3f}) ms {fl[v] / best[v] / 1e9:.0f} TF/s"
                          for v in forms))
            say(f"    ratios: a/b {best['a'] / best['b']:.3f}  a/b8 {best['a'] / best['b8']:.3f}  "
                f"a/c {best['a'] / best['c']:.3f}" + (f"  a/d {best['a'] / best['d']:.3f}" if "d" in best else ""))
            del a, w, w8, a8, sc, la, lb, t, b, gate, out
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
