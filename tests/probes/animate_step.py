"""Cost of Wan2.2-Animate at the 14B dims (dim 5120, 40 heads, 40 layers, in_dim 36, CLIP branch), 832x480x81
(latents 16 x 21 x 60 x 104: S = 32 760 tokens, 1 560 per latent frame), B = 2 (CFG), random weights as bench.py
builds them, T_face = 77 (21 frames of 5 motion tokens).

  (a) the whole CFG step under hipGraph replay with the adapter (pose rows + 8 fuser blocks) against the plain
      I2V step on the same tree: REPS interleaved replays, host clock around a synchronise;
  (b) vs_face_attn alone (in place, as the model runs it) in us and achieved GB/s (q read + o written + K / V
      once), and the unfused route on the same inputs: vs_head_rmsnorm in place + vs_attn_fwd at skv = 5,
      batch = B T;
  (c) the once-per-call preparation: pose rows, face encoder, the 8 K / V buffers.

  python tests/probes/animate_step.py [--reps 3] [--layers 40] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "video-styler_amd"))
import torch

from vstyler import kernels as K
from vstyler import model_fn_wan_video
from vstyler.flow_match import FlowMatchScheduler
from vstyler.models import WanAnimateAdapter, WanModel, Workspace, init_random_
from vstyler.pipeline import DenoiseStepper

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--layers", type=int, default=40)
ap.add_argument("--kernel-reps", type=int, default=20)
ap.add_argument("--skip-step", action="store_true", help="(b) and (c) only")
ap.add_argument("--out", default=None, help="also write the JSON record to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
BF16 = torch.bfloat16
D, HEADS, FFN = 5120, 40, 13824
T, Hl, Wl = 21, 60, 104
N = (Hl // 2) * (Wl // 2)
S = T * N
B, L, TF, NK = 2, 512, 77, 5
rec = {"S": S, "n": N, "B": B, "reps": args.reps, "layers": args.layers, "t_face": TF}
g = torch.Generator().manual_seed(1)


def summary(ms):
    v = sorted(ms)
    return {"ms": [round(x, 4) for x in ms], "median_ms": round(v[len(v) // 2], 4), "spread_ms": round(v[-1] - v[0], 4)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1000 * (time.perf_counter() - t0)


def event_us(fn, reps):
    """Median / spread of `reps` single launches between two events, after two warm-up launches."""
    fn(), fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(1000 * e0.elapsed_time(e1))
    v = sorted(out)
    return {"median_us": round(v[len(v) // 2], 1), "min_us": round(v[0], 1), "max_us": round(v[-1], 1)}


ad = init_random_(WanAnimateAdapter(dim=D, num_heads=HEADS, num_layers=args.layers, device=dev), seed=7)
ws = Workspace(dev)
pose = torch.randn(1, 16, T - 1, Hl, Wl, generator=g).to(BF16).to(dev)
motion = torch.randn(B, TF, 512, generator=g).to(BF16).to(dev)

# ---- (c) once per call
rec["prep_pose_rows"] = summary([timed(lambda: ad.pose_rows(pose, T, ws)) for _ in range(args.reps + 1)][1:])
rec["prep_face_encoder"] = summary([timed(lambda: ad.motion_tokens(motion, ws)) for _ in range(args.reps + 1)][1:])
mv = ad.motion_tokens(motion, ws)
assert tuple(mv.shape) == (B, T, NK, D), tuple(mv.shape)
rec["prep_face_kv"] = summary([timed(lambda: ad.face_kv(mv, ws)) for _ in range(args.reps + 1)][1:])
rec["prep_total_ms"] = round(sum(rec[k]["median_ms"] for k in ("prep_pose_rows", "prep_face_encoder", "prep_face_kv")), 3)
for k in ("prep_pose_rows", "prep_face_encoder", "prep_face_kv"):
    print(f"once per call, {k}: {rec[k]}", flush=True)
print(f"once per call, total: {rec['prep_total_ms']} ms", flush=True)

# ---- (b) the kernel alone
q0 = (2.0 * torch.randn(B * S, D, device=dev)).to(BF16)
kk = torch.randn(B, T * NK, D, generator=g).to(BF16).to(dev)
vv = torch.randn(B, T * NK, D, generator=g).to(BF16).to(dev)
wq = (1 + 0.1 * torch.randn(128, generator=g)).to(BF16).to(dev)
q = q0.clone()
geom = dict(batch=B, num_heads=HEADS, frames=T, tokens_per_frame=N, nkeys=NK)
fused = event_us(lambda: K.face_attn(q, kk, vv, wq, **geom), args.kernel_reps)
nbytes = 2 * q.numel() * 2 + 2 * kk.numel() * 2
fused["GBps"] = round(nbytes / (fused["median_us"] * 1e-6) / 1e9, 1)
rec["face_attn"] = fused
print(f"vs_face_attn [{B * S} x {D}], {NK} keys: {fused} ({nbytes / 1e9:.3f} GB moved)", flush=True)
o = torch.empty_like(q)
k2, v2 = kk.view(B * T * NK, D), vv.view(B * T * NK, D)
norm = event_us(lambda: K.head_rmsnorm(q, wq, HEADS), args.kernel_reps)
attn = event_us(lambda: K.attention(q, k2, v2, o, HEADS, B * T), args.kernel_reps)
rec["unfused"] = {"head_rmsnorm": norm, "attn_fwd_skv5": attn, "median_us": round(norm["median_us"] + attn["median_us"], 1)}
rec["fused_over_unfused"] = round(fused["median_us"] / rec["unfused"]["median_us"], 4)
print(f"unfused route: vs_head_rmsnorm {norm}, vs_attn_fwd (skv {NK}, batch {B * T}) {attn}: "
      f"{rec['unfused']['median_us']} us; fused / unfused = {rec['fused_over_unfused']}", flush=True)
del q, q0, o
torch.cuda.empty_cache()

# ---- (a) the step
if not args.skip_step:
    dit = init_random_(WanModel(dim=D, in_dim=36, ffn_dim=FFN, out_dim=16, text_dim=4096, freq_dim=256, eps=1e-6,
                                patch_size=(1, 2, 2), num_heads=HEADS, num_layers=args.layers, has_image_input=True,
                                device=dev), seed=5)
    ctx = 0.1 * torch.randn(2, L, 4096, generator=g)
    ctx[0, 32:] = 0
    ctx[1, 96:] = 0
    ctx = ctx.to(BF16).to(dev)
    clip = torch.randn(1, 257, 1280, generator=g).to(BF16).to(dev)
    y = torch.randn(1, 20, T, Hl, Wl, generator=g).to(BF16).to(dev)
    n_steps = 64
    sched = FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
    sched.set_timesteps(n_steps, shift=5.0)
    ts = sched.timesteps.to(BF16).to(dev)
    ds = torch.tensor([sched.delta(i) for i in range(n_steps)], dtype=torch.float32, device=dev)
    nxt = iter(range(n_steps))

    def stepper(stream=None, **const):
        latents = torch.randn(1, 16, T, Hl, Wl, generator=g).to(BF16).to(dev)

        def step_fn(t_buf, d_buf):
            v = model_fn_wan_video(dit, latents=latents, timestep=t_buf, context=ctx, y=y, clip_feature=clip, **const)
            K.cfg_euler_dev(v[0:1], v[1:2], latents, 5.0, d_buf)
        return DenoiseStepper(step_fn, ts, ds, use_graph=True, stream=stream)

    from vstyler.pipeline import _workspace
    pws = _workspace(dev)
    const = dict(animate_adapter=ad, pose_tokens=ad.pose_rows(pose, T, pws),
                 animate_kv=ad.face_kv(ad.motion_tokens(motion, pws), pws))
    st = {"plain": stepper()}
    st["animate"] = stepper(stream=st["plain"].stream, **const)
    for name, s in st.items():
        a = timed(lambda: s(next(nxt)))
        b = timed(lambda: s(next(nxt)))
        if s.graph is None:
            raise RuntimeError(f"{name}: the step was not captured")
        print(f"{name}: eager step + capture {a:.1f} ms, first replay {b:.1f} ms", flush=True)
    ms = {k: [] for k in st}
    for _ in range(args.reps):              # interleaved repeats
        for name, s in st.items():
            ms[name].append(timed(lambda: s(next(nxt))))
    for name in st:
        rec[f"step_{name}"] = summary(ms[name])
        print(f"step {name}: {rec[f'step_{name}']}", flush=True)
    rec["animate_over_plain"] = round(rec["step_animate"]["median_ms"] / rec["step_plain"]["median_ms"], 4)
    print(f"animate step: {rec['animate_over_plain']} x the plain I2V step "
          f"(+{rec['step_animate']['median_ms'] - rec['step_plain']['median_ms']:.1f} ms)", flush=True)

print(json.dumps(rec), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
