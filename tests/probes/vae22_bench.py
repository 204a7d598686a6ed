"""Probe: the Wan2.2 VAE (WanVideoVAE38, random weights) tiled encode / decode at 1280x704x121 -- the
TI2V-5B output size -- on one MI355X, tiles (30, 52) / (15, 26) latent units (480 x 832 pixels).
Prints per call: wall time, the algorithmic FLOPs counter, TFLOP/s, the allocator's peak, and the share of
GPU time per layer kind (events around every launch wrapper of vstyler.vae; "other" is the tile gather /
blend, the attention softmax / transpose, the frame copies and idle time between launches).
Usage: python tests/probes/vae22_bench.py   (VAE_T / VAE_H / VAE_W / VAE_REPS override the size)"""
import collections
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-styler_amd")]
import torch  # noqa: E402

from vstyler import vae  # noqa: E402

EVENTS = []


def _timed(label_of, fn):
    def run(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*a, **kw)
        e1.record()
        EVENTS.append((label_of(*a, **kw), e0, e1))
        return out
    return run


def _conv_kind(x, cw, out_thw, **kw):
    kt, kh, kw_ = cw.k
    if (kt, kh, kw_) == (3, 3, 3):
        return "conv 3x3x3"
    if (kt, kh, kw_) == (1, 1, 1):
        return "conv 1x1x1"
    if kt == 3:
        return "conv time 3x1x1"
    return "conv 3x3 up2" if kw.get("up2") else "conv 3x3 stride 2"


def instrument():
    vae.conv = _timed(_conv_kind, vae.conv)
    vae.batched_gemm = _timed(lambda *a, **k: "attention GEMMs", vae.batched_gemm)
    vae.rmsnorm = _timed(lambda *a, **k: "rmsnorm", vae.rmsnorm)
    vae.avgdown_add = _timed(lambda *a, **k: "avgdown_add", vae.avgdown_add)
    vae.dupup_add = _timed(lambda *a, **k: "dupup_add", vae.dupup_add)
    vae.patchify2 = _timed(lambda *a, **k: "patchify", vae.patchify2)
    vae.unpatchify2 = _timed(lambda *a, **k: "unpatchify", vae.unpatchify2)


def call(tag, fn):
    EVENTS.clear()
    vae.FLOPS[0] = 0
    torch.cuda.reset_peak_memory_stats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kinds = collections.OrderedDict()
    for label, e0, e1 in EVENTS:
        kinds[label] = kinds.get(label, 0.0) + e0.elapsed_time(e1) * 1e-3
    kinds["other"] = max(0.0, dt - sum(kinds.values()))
    print(f"{tag} {tuple(out.shape)} {dt:.3f} s  {vae.FLOPS[0] / 1e12:.1f} TFLOP  {vae.FLOPS[0] / dt / 1e12:.0f} TF/s  "
          f"peak mem {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB  launches {len(EVENTS)}", flush=True)
    print("    " + "  ".join(f"{k} {100 * v / dt:.1f}%" for k, v in sorted(kinds.items(), key=lambda kv: -kv[1])), flush=True)
    return out


def main():
    frames, H, W = int(os.environ.get("VAE_T", 121)), int(os.environ.get("VAE_H", 704)), int(os.environ.get("VAE_W", 1280))
    reps = int(os.environ.get("VAE_REPS", 1))
    m = vae.WanVideoVAE38(device="cuda").init_random_(seed=6)
    instrument()
    tile = dict(tiled=True, tile_size=(30, 52), tile_stride=(15, 26))
    print(f"WanVideoVAE38 {W}x{H}x{frames}, tiles per batch: encode {m._tile_batch(frames, 480, 832, False)}, "
          f"decode {m._tile_batch((frames - 1) // 4 + 1, 30, 52, True)} (tile_bytes {m.tile_bytes >> 30} GiB)", flush=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    video = (torch.rand((1, 3, frames, H, W), generator=g, device="cuda") * 2 - 1).to(torch.bfloat16)
    lat = None
    for it in range(reps + 1):
        lat = call(f"encode[{it}]", lambda: m.encode(video, "cuda", **tile))
    del video
    out = None
    for it in range(reps + 1):
        out = call(f"decode[{it}]", lambda: m.decode(lat, "cuda", **tile))
    u8 = vae.vae_output_to_u8(out[0])
    torch.cuda.synchronize()
    print("u8", tuple(u8.shape), f"mean {u8.float().mean().item():.2f}")


if __name__ == "__main__":
    main()
