"""Cost of image conditioning at the 14B dims, 832x480x81 (T' = 21, S = 32 760 tokens), B = 2 (CFG), random
weights as bench.py builds them, in_dim 36 with the image branch (the Wan2.1-I2V-14B layout).

(a) the cross-attention section of one block, per route of the image attention (host option
    img_attn_fused), HIP events around ITERS launches each, ROUNDS interleaved rounds:
      text_attn     K.attention over the 512 text keys (per-sample keys)
      img_kv_gemm   k_img | v_img of the 257 image rows, one GEMM (shared by both CFG samples)
      img_fused     K.attention_add over the 257 shared image keys (vs_attn_fwd_add)
      img_unfused   K.attention into a scratch buffer + K.axpy (the kernels that predate it)
    The two routes' outputs are compared bit for bit at this size (attn_nc=0, attn_impl=8 for the
    unfused attention).
(b) the whole CFG step (hipGraph replay) of the I2V model with y + clip_feature, per route, against the
    same-size T2V step (in_dim 16, no image branch), REPS interleaved repeats, host clock around a
    synchronise.

  python tests/probes/i2v_step.py [--rounds 3] [--iters 10] [--reps 3] [--layers 40] [--out FILE] [--skip-step]"""
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
from vstyler.models import WanModel, init_random_
from vstyler.options import host_options
from vstyler.pipeline import DenoiseStepper

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--layers", type=int, default=40)
ap.add_argument("--out", default=None, help="also write the JSON record to this file")
ap.add_argument("--skip-step", action="store_true", help="section (a) only")
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
BF16 = torch.bfloat16
D, HEADS, FFN = 5120, 40, 13824
T, Hl, Wl = 21, 480 // 8, 832 // 8
S = T * (Hl // 2) * (Wl // 2)
B, L, NI = 2, 512, 257
rec = {"S": S, "B": B, "rounds": args.rounds, "iters": args.iters, "reps": args.reps, "layers": args.layers}


def summary(ms):
    v = sorted(ms)
    return {"ms": [round(x, 4) for x in ms], "median_ms": round(v[len(v) // 2], 4), "spread_ms": round(v[-1] - v[0], 4)}


def events(fn, iters):
    """ms per call: HIP events around `iters` back-to-back launches."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def model(in_dim, image, seed):
    m = WanModel(dim=D, in_dim=in_dim, ffn_dim=FFN, out_dim=16, text_dim=4096, freq_dim=256, eps=1e-6,
                 patch_size=(1, 2, 2), num_heads=HEADS, num_layers=args.layers, has_image_input=image, device=dev)
    return init_random_(m, seed=seed)


def section_probe(dit):
    g = torch.Generator(device=dev).manual_seed(3)

    def rnd(*shape, scale=1.0):
        return (scale * torch.randn(shape, generator=g, device=dev)).to(BF16)
    q, o, oi = rnd(B * S, D), torch.empty(B * S, D, dtype=BF16, device=dev), torch.empty(B * S, D, dtype=BF16, device=dev)
    kv = rnd(B * L, 2 * D)
    img = rnd(NI, D)
    ca = dit.blocks[0].cross_attn
    kvi = torch.empty(NI, 2 * D, dtype=BF16, device=dev)
    K.gemm(img, ca._fw_img, kvi, bias=ca._fb_img)
    kvi.copy_(rnd(NI, 2 * D))               # N(0, 1) keys / values like the text ones
    kvi2 = torch.empty_like(kvi)
    routes = {
        "text_attn": lambda: K.attention(q, kv[:, :D], kv[:, D:], o, HEADS, B),
        "img_kv_gemm": lambda: K.gemm(img, ca._fw_img, kvi2, bias=ca._fb_img),
        "img_fused": lambda: K.attention_add(q, kvi[:, :D], kvi[:, D:], o, HEADS, B, shared_kv=True),
        "img_unfused": lambda: (K.attention(q, kvi[:, :D], kvi[:, D:], oi, HEADS, B, shared_kv=True), K.axpy(o, oi, 1.0)),
    }
    # same bits at this size: text attention into o, then each route
    K.attention(q, kv[:, :D], kv[:, D:], o, HEADS, B)
    base = o.clone()
    routes["img_fused"]()
    fused = o.clone()
    o.copy_(base)
    with K.options(attn_nc=0, attn_impl=8):
        routes["img_unfused"]()
    torch.cuda.synchronize()
    rec["routes_bit_identical"] = bool(torch.equal(fused.view(torch.int16), o.view(torch.int16)))
    print(f"fused == unfused bit for bit at B={B} S={S}: {rec['routes_bit_identical']}", flush=True)
    for fn in routes.values():              # warm every shape
        events(fn, 2)
    ms = {k: [] for k in routes}
    for _ in range(args.rounds):            # interleaved rounds
        for name, fn in routes.items():
            ms[name].append(events(fn, args.iters))
    for name in routes:
        rec[name] = summary(ms[name])
        print(f"{name}: {rec[name]}", flush=True)
    d = [f - u for f, u in zip(ms["img_fused"], ms["img_unfused"])]
    rec["fused_minus_unfused_ms"] = [round(x, 4) for x in d]
    rec["round_spread_ms"] = round(max(rec["img_fused"]["spread_ms"], rec["img_unfused"]["spread_ms"]), 4)
    print(f"fused - unfused per round: {rec['fused_minus_unfused_ms']} ms (spread between rounds "
          f"{rec['round_spread_ms']} ms)", flush=True)


def step_probe(i2v):
    t2v = model(16, False, 9)
    g = torch.Generator().manual_seed(1)
    ctx = 0.1 * torch.randn(2, L, 4096, generator=g)
    ctx[0, 32:] = 0
    ctx[1, 96:] = 0
    ctx = ctx.to(BF16).to(dev)
    y = torch.randn(1, 20, T, Hl, Wl, generator=g).to(BF16).to(dev)
    clip = torch.randn(1, NI, 1280, generator=g).to(BF16).to(dev)
    n_steps = 64
    sched = FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
    sched.set_timesteps(n_steps, shift=5.0)
    ts = sched.timesteps.to(BF16).to(dev)
    ds = torch.tensor([sched.delta(i) for i in range(n_steps)], dtype=torch.float32, device=dev)
    nxt = iter(range(n_steps))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1000 * (time.perf_counter() - t0)

    def stepper(dit, fused, stream=None, **kw):
        latents = torch.randn(1, 16, T, Hl, Wl, generator=g).to(BF16).to(dev)

        def step_fn(t_buf, d_buf):
            with host_options(img_attn_fused=fused):
                v = model_fn_wan_video(dit, latents=latents, timestep=t_buf, context=ctx, **kw)
            K.cfg_euler_dev(v[0:1], v[1:2], latents, 5.0, d_buf)
        return DenoiseStepper(step_fn, ts, ds, use_graph=True, stream=stream)

    steppers = {"t2v": stepper(t2v, 0)}
    steppers["i2v_unfused"] = stepper(i2v, 0, stream=steppers["t2v"].stream, y=y, clip_feature=clip)
    steppers["i2v_fused"] = stepper(i2v, 1, stream=steppers["t2v"].stream, y=y, clip_feature=clip)
    for name, st in steppers.items():
        first = timed(lambda: st(next(nxt)))
        replay = timed(lambda: st(next(nxt)))
        if st.graph is None:
            raise RuntimeError(f"{name}: the step was not captured")
        print(f"{name}: eager step + capture {first:.1f} ms, first replay {replay:.1f} ms", flush=True)
    ms = {k: [] for k in steppers}
    for _ in range(args.reps):              # interleaved repeats
        for name, st in steppers.items():
            ms[name].append(timed(lambda: st(next(nxt))))
    for name in steppers:
        rec["step_" + name] = summary(ms[name])
        print(f"step {name}: {rec['step_' + name]}", flush=True)
    t = rec["step_t2v"]["median_ms"]
    for name in ("i2v_unfused", "i2v_fused"):
        rec[name + "_over_t2v"] = round(rec["step_" + name]["median_ms"] / t, 4)
    print(f"image conditioning: unfused {rec['i2v_unfused_over_t2v']} x, fused {rec['i2v_fused_over_t2v']} x the T2V "
          f"step", flush=True)


i2v = model(36, True, 5)
section_probe(i2v)
if not args.skip_step:
    step_probe(i2v)
print(json.dumps(rec), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
