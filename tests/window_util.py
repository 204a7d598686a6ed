"""Test-side temporal tiler: TemporalTiler_BCTHW.run (diffsynth/pipelines/wan_video_new.py:1207-1256)
restated literally with torch tensor ops around any forward function, with the one deviation of this
build -- vace_context is cut with the same [t, t_) as the latents.  Never used by the product path."""
import torch


def build_1d_mask(length, left_bound, right_bound, border_width):
    x = torch.ones((length,))
    if border_width == 0:
        return x
    shift = 0.5
    if not left_bound:
        x[:border_width] = (torch.arange(border_width) + shift) / border_width
    if not right_bound:
        x[-border_width:] = torch.flip((torch.arange(border_width) + shift) / border_width, dims=(0,))
    return x


def tile(forward, latents, vace_context, sliding_window_size, sliding_window_stride):
    """forward(latents[:, :, t:t_], vace_context[:, :, t:t_] or None) -> [B, C, t_ - t, H, W]; the
    blend runs on the outputs' device in their dtype, as the reference's does."""
    T = latents.shape[2]
    value, weight = None, None
    for t in range(0, T, sliding_window_stride):
        if t - sliding_window_stride >= 0 and t - sliding_window_stride + sliding_window_size >= T:
            continue
        t_ = min(t + sliding_window_size, T)
        model_output = forward(latents[:, :, t: t_], None if vace_context is None else vace_context[:, :, t: t_])
        if value is None:
            B, C, _, H, W = model_output.shape
            value = torch.zeros((B, C, T, H, W), device=model_output.device, dtype=model_output.dtype)
            weight = torch.zeros((1, 1, T, 1, 1), device=model_output.device, dtype=model_output.dtype)
        mask = build_1d_mask(t_ - t, t == 0, t_ == T, sliding_window_size - sliding_window_stride)
        mask = mask.reshape(1, 1, -1, 1, 1).to(device=value.device, dtype=value.dtype)
        value[:, :, t: t_, :, :] += model_output * mask
        weight[:, :, t: t_, :, :] += mask
    value /= weight
    return value


def tiled_model_fn(plain):
    """A stand-in for WanVideoPipeline.model_fn: takes the call the pipeline makes, runs `plain` (the
    product model_fn_wan_video without the window arguments) under the test-side tiler."""
    def fn(**kw):
        size, stride = kw.pop("sliding_window_size"), kw.pop("sliding_window_stride")
        kw.pop("vace_context_windows", None)
        latents, vace_context = kw.pop("latents"), kw.pop("vace_context", None)
        return tile(lambda lat, vc: plain(latents=lat, vace_context=vc, **kw), latents, vace_context, size, stride)
    return fn
