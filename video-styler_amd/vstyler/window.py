"""Host plan of the temporal sliding window (TemporalTiler_BCTHW, diffsynth/pipelines/
wan_video_new.py:1207-1256): which windows of the latent time axis a denoising step runs, each
window's blend mask and the accumulated weight, all in the reference's arithmetic.  Pure torch on the
CPU: usable without a GPU.

Units are latent frames (the T axis of the [B, 16, T, h, w] latents, prepended reference frames
included)."""
from dataclasses import dataclass
from typing import List, Tuple

import torch

BF16 = torch.bfloat16


def check_window_args(size, stride):
    """The two arguments as model_fn_wan_video takes them -> (size, stride) or None (no windows).
    stride alone is ignored, as in the reference (:1291); size alone, non-ints and anything outside
    1 <= stride <= size are ValueErrors (the reference would loop forever or fail in the mask
    assignment)."""
    if size is None:
        return None
    if stride is None:
        raise ValueError("sliding_window_size needs sliding_window_stride")
    for name, v in (("sliding_window_size", size), ("sliding_window_stride", stride)):
        if not isinstance(v, int) or isinstance(v, bool):
            raise ValueError(f"{name} must be an int (latent frames), got {v!r}")
    if not 1 <= stride <= size:
        raise ValueError(f"need 1 <= sliding_window_stride <= sliding_window_size, got stride {stride}, size {size}")
    return size, stride


def window_list(T, size, stride) -> List[Tuple[int, int]]:
    """The [t, t_) windows of :1238-1241."""
    wins = []
    for t in range(0, T, stride):
        if t - stride >= 0 and t - stride + size >= T:
            continue
        wins.append((t, min(t + size, T)))
    return wins


def window_mask(length, left_bound, right_bound, border_width):
    """build_1d_mask (:1211-1221) rounded to bf16 (:1251): fp32 ones, a linear ramp of border_width
    frames on every side that is not a clip boundary; the right ramp is assigned last and overwrites
    the left one where they overlap."""
    x = torch.ones((length,))
    if border_width == 0:
        return x.to(BF16)
    if not left_bound:
        x[:border_width] = (torch.arange(border_width) + 0.5) / border_width
    if not right_bound:
        x[-border_width:] = torch.flip((torch.arange(border_width) + 0.5) / border_width, dims=(0,))
    return x.to(BF16)


@dataclass
class WindowPlan:
    T: int
    size: int
    stride: int
    windows: List[Tuple[int, int]]
    masks: List[torch.Tensor]       # per window: bf16 [t_ - t]
    weight: torch.Tensor            # bf16 [T]: the masks accumulated in bf16, window by window (:1253)


def plan_windows(T, size, stride) -> WindowPlan:
    size, stride = check_window_args(size, stride)
    if not isinstance(T, int) or T < 1:
        raise ValueError(f"T must be a positive int, got {T!r}")
    wins = window_list(T, size, stride)
    masks = [window_mask(t_ - t, t == 0, t_ == T, size - stride) for t, t_ in wins]
    weight = torch.zeros((T,), dtype=BF16)
    for (t, t_), m in zip(wins, masks):
        weight[t:t_] += m
    return WindowPlan(T, size, stride, wins, masks, weight)
