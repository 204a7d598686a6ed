"""Two-expert denoising (Wan2.2 A14B: a high-noise and a low-noise DiT): the host-side plan every
sampling loop follows, the per-expert guidance scale, and the nearest-neighbour source index of the
enhancer's frame resize.  Pure host arithmetic, no device call.

Reference: diffsynth/pipelines/wan_video_new.py:518-523 (the switch), denoising_enhancing/wan/
text2video.py:384-385 (the guidance pair).
"""
import numbers

import numpy as np

NUM_TRAIN_TIMESTEPS = 1000


def plan_experts(timesteps, boundary, has_second):
    """Contiguous segments [(first, last, expert)] (step indices, both ends inclusive; expert 1 or 2)
    covering steps 0 .. len(timesteps) - 1.  Step i runs on expert 2 iff a second expert exists and
    float(timesteps[i]) < boundary * 1000, compared on the scheduler's own fp32 / int64 value (before
    any bf16 cast); the switch is sticky, as the reference's `models["dit"] = self.dit2` is: once a
    step has selected expert 2 every later step stays on it."""
    ts = [float(t) for t in timesteps]
    if not ts:
        return []
    segs, first, cur = [], 0, 1
    for i, t in enumerate(ts):
        e = 2 if has_second and (cur == 2 or t < float(boundary) * NUM_TRAIN_TIMESTEPS) else 1
        if e != cur:
            if i > first:
                segs.append((first, i - 1, cur))
            first, cur = i, e
    segs.append((first, len(ts) - 1, cur))
    return segs


def _is_number(x):
    return isinstance(x, numbers.Real) and not isinstance(x, bool)


def expert_cfg_scales(cfg_scale, has_second):
    """(scale of expert 1, scale of expert 2).  cfg_scale is one number for both, or the enhancer's
    (low_noise, high_noise) pair: expert 1 (`dit`, high noise) takes [1], expert 2 takes [0]."""
    if _is_number(cfg_scale):
        return float(cfg_scale), float(cfg_scale)
    if isinstance(cfg_scale, (tuple, list)) and len(cfg_scale) == 2 and all(_is_number(c) for c in cfg_scale):
        if not has_second:
            raise ValueError("a (low_noise, high_noise) cfg_scale pair needs a second expert (dit2)")
        return float(cfg_scale[1]), float(cfg_scale[0])
    raise ValueError(f"cfg_scale must be a number or a (low_noise, high_noise) pair of numbers, got {cfg_scale!r}")


def nearest_index(n_in, n_out):
    """Source index of every destination index of a nearest-neighbour resize of one axis, as
    F.interpolate(mode="nearest") and vs_resize_nearest_u8 compute it in fp32:
    min(floor(dst * (float(n_in) / float(n_out))), n_in - 1) -> int32 array [n_out]."""
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int32)
    return np.minimum(src, n_in - 1)
