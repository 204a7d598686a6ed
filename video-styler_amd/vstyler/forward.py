"""model_fn_wan_video (diffsynth/pipelines/wan_video_new.py:1260-1468) on libvstyler kernels: the support
matrix of its features, the record of what rides along a forward, and the forward itself as four steps --
check, build the record, dispatch (windows, then the y / clip gating, then the CFG-parallel split), the plain
forward."""
import dataclasses
import functools

import torch

from . import kernels as K
from .models import IMG_TOKENS, RunCtx, Workspace, WanModel, VaceWanModel
from .window import check_window_args, plan_windows

BF16 = torch.bfloat16

_WS = {}


def _workspace(device):
    key = str(torch.device(device))
    if key not in _WS:
        _WS[key] = Workspace(device)
    return _WS[key]


_UNSUPPORTED = ("audio_embeds", "motion_latents", "s2v_pose_latents", "motion_bucket_id")

# ---------------------------------------------------------------------------------------- the support matrix
# feature -> its name in a message
FEATURES = {
    "animate": "the animate adapter (pose_latents / animate_face_motion)",
    "first_frame": "fuse_vae_embedding_in_latents (first_frame_latents)",
    "windows": "a temporal sliding window of more than one window",
    "tea_cache": "tea_cache (tea_cache_l1_thresh)",
    "vace": "a VACE context",
    "reference": "reference_latents",
    "camera": "camera control",
    "slg": "slg_blocks",
    "sp": "Ulysses / CFG parallelism",
    "dit2": "a second expert (dit2)",
}

# (feature, what it does not run with), rows and columns in reporting order
EXCLUDES = (
    ("animate", ("windows", "tea_cache", "dit2", "vace", "reference", "first_frame", "camera", "slg")),
    # the first-frame segment: two modulation rows per sample, one timestep for the batch
    ("first_frame", ("sp", "windows", "tea_cache", "vace", "dit2")),
    # the reference hands one TeaCache state to every window (:1304), which compares and reuses residuals
    # across different windows; its tiler drops the camera input (:1292-1307)
    ("windows", ("tea_cache", "camera")),
    # the reference hands one TeaCache state to both experts and has no coefficients for them
    ("dit2", ("tea_cache",)),
)


def check_support(features, who):
    """features: {key of FEATURES: whether the call uses it}.  NotImplementedError for the first pair of
    EXCLUDES whose two features are both in use; `who` (the caller) leads the message."""
    names = {key: FEATURES[key] for key, on in features.items() if on}      # (KeyError: not a feature)
    for feature, excluded in EXCLUDES:
        for other in excluded:
            if feature in names and other in names:
                raise NotImplementedError(f"{who}: {names[feature]} with {names[other]} is not supported")


# ------------------------------------------------------------------------------------------------ windows
_WINDOW_PLANS = {}


def _device_plan(device, plan):
    """The masks and the weight of a host plan on `device`, copied once per (device, T, size, stride)."""
    key = (str(torch.device(device)), plan.T, plan.size, plan.stride)
    if key not in _WINDOW_PLANS:
        _WINDOW_PLANS[key] = ([m.to(device) for m in plan.masks], plan.weight.to(device))
    return _WINDOW_PLANS[key]


def slice_windows(x, plan):
    """x[:, :, t:t_] of every window of the plan as contiguous bf16 tensors: what a caller that runs
    many steps on one vace_context hands to model_fn_wan_video(vace_context_windows=)."""
    x = x.to(BF16).contiguous()
    B, C, T, H, W = x.shape
    return [K.window_gather(x, t, torch.empty((B, C, t_ - t, H, W), device=x.device, dtype=BF16))
            for t, t_ in plan.windows]


# ------------------------------------------------------------------------------------------------ the record
def _mine(tn, c):
    """CFG-parallel rank c's sample of a batch-2 tensor, or of every tensor of a list; a batch-1 (shared)
    tensor passes."""
    if isinstance(tn, list):
        return [_mine(x, c) for x in tn]
    return tn[c:c + 1] if tn is not None and tn.dim() > 0 and tn.shape[0] == 2 else tn


def _rides(sample, window="pass"):
    """A Conditioning field with its two rules.  sample: "batch" ([1 or 2, ...], or a list of such), "frame_rows" /
    "rows" (token rows [per or 2 per, D] of one latent frame / of all), "whole".  window: "pass", or the workspace
    buffer a [B, C, T, H, W] tensor is cut into unless its pre-cut list (the field NAME_windows) is there."""
    return dataclasses.field(default=None, metadata={"sample": sample, "window": window})


@dataclasses.dataclass
class Conditioning:
    """What rides along one forward beside latents, timestep and context, each input raw and / or precomputed
    (the precomputed form wins).  sample() and window() are the only two places that split a forward, and both
    walk dataclasses.fields: a field without a rule is a TypeError there, never a silently dropped input."""
    y: torch.Tensor = _rides("batch", "win_y")
    y_windows: list = _rides("batch")
    clip_feature: torch.Tensor = _rides("batch")
    vace_context: torch.Tensor = _rides("batch", "win_vace")
    vace_context_windows: list = _rides("batch")
    reference_latents: torch.Tensor = _rides("batch")
    reference_tokens: torch.Tensor = _rides("frame_rows")
    control_camera_latents_input: torch.Tensor = _rides("whole")
    camera_tokens: torch.Tensor = _rides("rows")
    pose_latents: torch.Tensor = _rides("batch")
    pose_tokens: torch.Tensor = _rides("rows")
    animate_face_motion: torch.Tensor = _rides("batch")
    animate_kv: list = _rides("batch")

    @classmethod
    @functools.lru_cache(maxsize=None)
    def _rules(cls, which):
        """((field, its `which` rule), ...) over dataclasses.fields, read once per class (a forward splits per step)."""
        missing = [f.name for f in dataclasses.fields(cls) if which not in f.metadata]
        if missing:
            raise TypeError(f"{cls.__name__}: {missing} have no '{which}' rule: they would not ride a split forward")
        return tuple((f.name, f.metadata[which]) for f in dataclasses.fields(cls))

    def _each(self, which, rule):
        return type(self)(**{name: rule(name, how, getattr(self, name)) for name, how in self._rules(which)})

    def sample(self, c, hw, frames):
        """CFG-parallel rank c's view (c = 0 / 1) of a batch-2 forward over `frames` latent frames of hw tokens:
        per-sample forms are cut to sample c, shared forms (batch 1, rows of one sample) are the same objects."""
        def rule(name, how, v):
            if v is None or how == "whole":
                return v
            if how == "batch":
                return _mine(v, c)
            if how in ("frame_rows", "rows"):       # [2 per, D] -> [per, D]
                per = hw if how == "frame_rows" else frames * hw
                return v if v.shape[0] == per else v[c * per:(c + 1) * per]
            raise TypeError(f"Conditioning.{name}: unknown sample rule {how!r}")
        return self._each("sample", rule)

    def window(self, i, t, t_, ws):
        """Window i's view, latent frames [t, t_): y and vace_context (contiguous bf16) are cut by vs_window_gather
        into their workspace buffers or taken from the pre-cut lists; everything else passes (the lists too: a plain
        forward does not look at them)."""
        def rule(name, how, v):
            if how == "pass":
                return v
            pre = getattr(self, name + "_windows")
            if pre is not None:
                return pre[i]
            if v is None:
                return None
            return K.window_gather(v, t, ws.get(how, (v.shape[0], v.shape[1], t_ - t) + tuple(v.shape[3:])))
        return self._each("window", rule)


# ------------------------------------------------------------------------------------ per-input validation
def _encode_face_pixels(adapter, pixels, motion, kv):
    """model_fn's face_pixel_values [B, 3, T_face, size, size] -> animate_face_motion [B, T_face, 512] through the
    adapter's motion encoder, sample by sample (after_patch_embedding, wan_video_animate_adapter.py:627-637)."""
    size = None if adapter is None else adapter.motion_size()
    if size is None:
        raise NotImplementedError("model_fn_wan_video: 'face_pixel_values' needs animate_adapter= with the complete "
                                  "motion-encoder weights (motion_encoder.*): pass the motion vectors as "
                                  "animate_face_motion=")
    if motion is not None or kv is not None:
        raise ValueError("model_fn_wan_video: pass face_pixel_values or its motion vectors (animate_face_motion / "
                         "animate_kv), not both")
    if pixels.dim() != 5 or pixels.shape[1] != 3 or tuple(pixels.shape[3:]) != (size, size):
        raise ValueError(f"model_fn_wan_video: face_pixel_values {tuple(pixels.shape)}: expected [B, 3, T_face, {size}, "
                         f"{size}] (the motion encoder's size; the reference does not resize either)")
    return torch.stack([adapter.encode_motion(p.to(BF16)) for p in pixels])


def _reference_frame(reference_latents, latents, batch):
    """reference_latents [1 or B, 16, (1,) H, W] as a [Br, 16, H, W] tensor (wan_video_new.py:1386-1387)."""
    r = reference_latents
    if r.dim() == 5 and r.shape[2] == 1:
        r = r[:, :, 0]
    want = (16,) + tuple(latents.shape[3:])
    if r.dim() != 4 or tuple(r.shape[1:]) != want or r.shape[0] not in (1, batch):
        raise ValueError(f"model_fn_wan_video: reference_latents {tuple(reference_latents.shape)}: expected "
                         f"[1 or {batch}, 16, (1,) {want[1]}, {want[2]}]")
    return r


def _check_camera_input(dit, cc, latents):
    T, H, W = latents.shape[2:]
    want = (1, dit.control_adapter.in_dim, T, 8 * H, 8 * W)
    if tuple(cc.shape) != want:
        raise ValueError(f"model_fn_wan_video: control_camera_latents_input {tuple(cc.shape)}: expected {want}")


def reference_token_rows(dit, reference_latents):
    """dit.ref_conv's tokens of reference_latents [Br, 16, (1,) H, W] as a tensor of their own
    [Br (H/2)(W/2), D]: what a denoising loop computes once and hands to every step as
    model_fn_wan_video(reference_tokens=)."""
    r = reference_latents[:, :, 0] if reference_latents.dim() == 5 else reference_latents
    dev = dit.ref_conv.weight.device
    return dit.ref_tokens(r.to(dev), _workspace(dev)).clone()


def camera_token_rows(dit, control_camera_latents_input, batch=1):
    """dit.control_adapter's output rows [S, D] replicated to [batch S, D]: computed once per call, the
    residual of every step's patch-embedding GEMM (model_fn_wan_video(camera_tokens=))."""
    rows = dit.control_adapter(control_camera_latents_input)
    return rows if batch == 1 else rows.repeat(batch, 1)


# ---------------------------------------------------------------------------------------------- the forward
def model_fn_wan_video(dit: WanModel, motion_controller=None, vace: VaceWanModel = None, animate_adapter=None,
                       latents: torch.Tensor = None, timestep: torch.Tensor = None, context: torch.Tensor = None,
                       vace_context=None, vace_scale=1.0, use_unified_sequence_parallel: bool = False,
                       sp_group=None, slg_blocks=(), tea_cache=None, cfg_sample=0, sliding_window_size=None,
                       sliding_window_stride=None, vace_context_windows=None, y=None, clip_feature=None,
                       y_windows=None, fuse_vae_embedding_in_latents=False, reference_latents=None,
                       control_camera_latents_input=None, reference_tokens=None, camera_tokens=None,
                       pose_latents=None, pose_tokens=None, animate_face_motion=None, animate_kv=None, **kwargs):
    """One DiT(+VACE) forward (wan_video_new.py:1338-1468) -> [B,dit.out_dim,T,H,W] bf16 velocity.

    `context` is [B, L, text_dim]; latents/timestep/vace_context with batch 1 are broadcast to B
    (the cfg_merge convention of wan_video_new.py:1361-1364).

    What does not run together is one table, EXCLUDES (check_support): NotImplementedError, raised here before
    any input is validated or anything is computed.

    fuse_vae_embedding_in_latents (with dit.seperated_timestep: Wan2.2-TI2V-5B's image-to-video mode,
    :1339-1349): latent frame 0 holds the clean first-frame latents and is modulated with timestep 0
    (_plain_forward).  One timestep for the whole batch, as the reference.

    slg_blocks: skip-layer guidance (config 5, ComfyUI WanVideoSLG): the listed main blocks are
    skipped for CFG sample 1 (the unconditional pass), run for sample 0 only.  cfg_sample: which
    CFG sample a batch-1 forward computes (1: it skips the slg_blocks) -- set by the CFG-parallel
    split (_gated_forward), which sp_group selects when it is a vstyler.usp.CfgParallel.

    sliding_window_size / sliding_window_stride (latent frames, both ints, 1 <= stride <= size): the
    temporal sliding window of wan_video_new.py:1291-1315 (_windowed_forward).  stride alone is
    ignored, as in the reference.  One window (size >= T) takes the plain path.  vace_context_windows:
    the vace_context already cut per window (slice_windows), so a denoising loop gathers it once.

    Image conditioning (wan_video_new.py:1366-1371; _gated_forward, _plain_forward).  y [1 or B, dit.in_dim - 16,
    T, H, W]: the mask + VAE-encoded image channels (y_windows: y pre-cut per window).  clip_feature [1 or B,
    257 or 514, 1280]: CLIP image features.

    Wan-Fun control.  reference_latents [1 or B, 16, (1,) H, W] on a has_ref_conv DiT (:1384-1390, :1463-1466)
    and control_camera_latents_input [1, 24, T, 8 H, 8 W] on a DiT with control_adapter (wan_video_dit.py
    :339-345).  Neither depends on the timestep: a denoising loop computes them once (reference_token_rows,
    camera_token_rows) and hands them over as reference_tokens [Br n, D] / camera_tokens [S or B S, D], which
    win over the raw inputs.  ValueError: a DiT without the module, a wrong shape, reference_latents together
    with a VACE context (the reference's token counts do not match there).

    Wan2.2-Animate (animate_adapter: a WanAnimateAdapter of the DiT's width).  pose_latents [1 or B, 16,
    T - 1, H, W] and animate_face_motion [1 or B, T_face, 512], the motion vectors of the face frames (the
    reference's motion_encoder.get_motion output).  Neither depends on the timestep: a denoising loop computes
    them once (WanAnimateAdapter.pose_rows, WanAnimateAdapter.face_kv) and hands them over as pose_tokens
    [S or B S, D] / animate_kv (one [B, T N, 2 D] buffer per fuser block), which win over the raw inputs.
    face_pixel_values [B, 3, T_face, size, size] (the reference's input, in [-1, 1]) is encoded per sample by
    the adapter's motion encoder (encode_motion) and proceeds as animate_face_motion; it excludes
    animate_face_motion / animate_kv, frames of another size are a ValueError, and without an adapter that
    holds the complete motion_encoder.* weights it is NotImplementedError."""
    face_pixel_values = kwargs.pop("face_pixel_values", None)
    win = check_window_args(sliding_window_size, sliding_window_stride)
    plan = None if win is None else plan_windows(latents.shape[2], *win)     # the forward's one plan
    windows = plan is not None and len(plan.windows) > 1
    animate = any(v is not None for v in (pose_latents, pose_tokens, animate_face_motion, animate_kv,
                                          face_pixel_values))
    seg = bool(fuse_vae_embedding_in_latents) and bool(dit.seperated_timestep)
    use_ref = reference_latents is not None or reference_tokens is not None
    use_cam = control_camera_latents_input is not None or camera_tokens is not None
    # (first_frame: the flag does nothing on a DiT without the segment, but the animate path refuses the flag itself)
    check_support({"animate": animate, "first_frame": seg or (animate and bool(fuse_vae_embedding_in_latents)),
                   "windows": windows, "tea_cache": tea_cache is not None, "reference": use_ref, "camera": use_cam,
                   "vace": vace is not None and vace_context is not None, "slg": len(slg_blocks) > 0,
                   "sp": bool(use_unified_sequence_parallel)}, "model_fn_wan_video")
    if face_pixel_values is not None:
        animate_face_motion = _encode_face_pixels(animate_adapter, face_pixel_values, animate_face_motion, animate_kv)
    if animate:
        if animate_adapter is None:
            raise ValueError("model_fn_wan_video: pose_latents / animate_face_motion need animate_adapter= (a "
                             "WanAnimateAdapter)")
        if animate_adapter.dim != dit.dim or animate_adapter.num_heads != dit.num_heads or \
                len(animate_adapter.face_adapter.fuser_blocks) != -(-len(dit.blocks) // 5):
            raise ValueError("model_fn_wan_video: the animate adapter's dim, num_heads or fuser block count do not "
                             "match the DiT")
    if use_ref:
        if not getattr(dit, "has_ref_conv", False):
            raise ValueError("model_fn_wan_video: reference_latents needs a DiT with ref_conv (has_ref_conv)")
        if vace is not None and vace_context is not None:
            raise ValueError("model_fn_wan_video: reference_latents together with a VACE context (the reference "
                             "tokens have no VACE rows)")
        if reference_tokens is None:
            reference_latents = _reference_frame(reference_latents, latents, context.shape[0])
    if use_cam:
        if getattr(dit, "control_adapter", None) is None:
            raise ValueError("model_fn_wan_video: control_camera_latents_input needs a DiT with control_adapter "
                             "(add_control_adapter)")
        if camera_tokens is None:
            _check_camera_input(dit, control_camera_latents_input, latents)
    for name in _UNSUPPORTED:
        if kwargs.get(name) is not None:
            raise NotImplementedError(f"model_fn_wan_video: '{name}' is outside the Ditto hot path")
    if seg and timestep.numel() != 1:
        raise ValueError("model_fn_wan_video: fuse_vae_embedding_in_latents takes one timestep for the batch")
    if vace is None:            # a VACE context without its module is not looked at
        vace_context = vace_context_windows = None
    cond = Conditioning(y=y, y_windows=y_windows, clip_feature=clip_feature, vace_context=vace_context,
                        vace_context_windows=vace_context_windows, reference_latents=reference_latents,
                        reference_tokens=reference_tokens, control_camera_latents_input=control_camera_latents_input,
                        camera_tokens=camera_tokens, pose_latents=pose_latents, pose_tokens=pose_tokens,
                        animate_face_motion=animate_face_motion, animate_kv=animate_kv)
    sp = sp_group if use_unified_sequence_parallel else None
    if use_unified_sequence_parallel and sp is None:
        from .usp import get_default_group
        sp = get_default_group()
    fwd = dict(dit=dit, vace=vace, animate_adapter=animate_adapter, timestep=timestep, context=context,
               vace_scale=vace_scale, sp=sp, slg_blocks=slg_blocks, cfg_sample=cfg_sample, tea_cache=tea_cache,
               seg=seg)
    if windows:
        return _windowed_forward(plan, latents, cond, **fwd)
    return _gated_forward(latents, cond, **fwd)


def _windowed_forward(plan, latents, cond, **fwd):
    """TemporalTiler_BCTHW.run (wan_video_new.py:1229-1256) around the forward: every window
    [t, t_) of the latent time axis is an ordinary forward of latents[:, :, t:t_] (RoPE positions
    0..t_-t-1, same timestep and context), blended into `value` with the window's mask and divided by
    the accumulated weight at the end, in the reference's bf16 arithmetic (vs_window_blend /
    vs_window_finish).  Unlike the reference, whose tiler slices only latents and y, vace_context is
    cut with the same [t, t_): a full-length context does not match the window's tokens.  y (the image
    conditioning channels) is cut per window as the reference's tiler does (its tensor_names list y),
    or comes pre-cut as y_windows (Conditioning.window)."""
    device = latents.device
    ws = _workspace(device)
    lat = latents.to(BF16).contiguous()
    Bl, C, T, H, W = lat.shape
    masks, weight = _device_plan(device, plan)
    if cond.reference_tokens is None and cond.reference_latents is not None:
        # the same reference rows in front of every window
        cond = dataclasses.replace(cond, reference_tokens=reference_token_rows(fwd["dit"], cond.reference_latents))
    if cond.vace_context is not None and cond.vace_context_windows is None:
        cond = dataclasses.replace(cond, vace_context=cond.vace_context.to(BF16).contiguous())
    if cond.y is not None and cond.y_windows is None:
        cond = dataclasses.replace(cond, y=cond.y.to(BF16).contiguous())
    value = None
    for i, (t, t_) in enumerate(plan.windows):
        lw = K.window_gather(lat, t, ws.get("win_lat", (Bl, C, t_ - t, H, W)))
        out = _gated_forward(lw, cond.window(i, t, t_, ws), **fwd)
        if value is None:
            value = torch.zeros((out.shape[0], out.shape[1], T, H, W), device=device, dtype=BF16)
        K.window_blend(out, masks[i], value, t)
    return K.window_finish(value, weight)


def _gated_forward(latents, cond, **fwd):
    """The image inputs against the DiT, then the CFG-parallel split (fwd: _plain_forward's keywords).

    y is concatenated behind the latents when dit.require_vae_embedding, and clip_feature is embedded by
    dit.img_emb when dit.require_clip_embedding and dit.has_image_input; otherwise each is dropped, as the
    reference does.  A DiT with in_dim > 16 needs y and one with has_image_input needs clip_feature: ValueError
    otherwise (the reference would feed the patch embedding too few channels / attend to the first 257 text
    rows as the image).

    sp_group may be a vstyler.usp.CfgParallel: a batch-2 (CFG) forward then runs as this rank's
    sample only (batch 1, Ulysses over its half of the ranks; Conditioning.sample) and the two samples'
    outputs are all-gathered across the halves -- the same [2,16,T,H,W] as the batched forward."""
    dit, context = fwd["dit"], fwd["context"]
    if cond.y is not None and not dit.require_vae_embedding:
        cond = dataclasses.replace(cond, y=None, y_windows=None)
    if cond.clip_feature is not None and not (dit.require_clip_embedding and dit.has_image_input):
        cond = dataclasses.replace(cond, clip_feature=None)
    if dit.has_image_input and cond.clip_feature is None:
        raise ValueError("model_fn_wan_video: this DiT has the image cross-attention branch (has_image_input): "
                         "pass clip_feature= (the CLIP image features, [1 or B, 257 or 514, 1280])")
    if cond.y is not None and 16 + cond.y.shape[1] != dit.in_dim:
        raise ValueError(f"model_fn_wan_video: y has {cond.y.shape[1]} channels, the DiT's patch embedding takes "
                         f"16 + {dit.in_dim - 16}")
    if cond.y is None and dit.in_dim > 16 and not dit.fuse_vae_embedding_in_latents:
        raise ValueError(f"model_fn_wan_video: the DiT's patch embedding takes {dit.in_dim} channels: pass y= "
                         f"({dit.in_dim - 16} image-conditioning channels)")
    plan = fwd["sp"]
    if plan is not None:
        from .usp import CfgParallel
        if isinstance(plan, CfgParallel):
            if context.shape[0] != 2 or fwd["tea_cache"] is not None:
                fwd["sp"] = plan.full           # no CFG pair to split (or a TeaCache step): Ulysses over all
            else:
                c = plan.cfg_rank
                hw = (latents.shape[3] // 2) * (latents.shape[4] // 2)
                mine = dict(fwd, timestep=_mine(fwd["timestep"].reshape(-1), c), context=context[c:c + 1],
                            sp=plan.ulysses, cfg_sample=c)
                local = _plain_forward(_mine(latents, c), cond.sample(c, hw, latents.shape[2]), **mine)
                out = torch.empty((2,) + tuple(local.shape[1:]), device=local.device, dtype=local.dtype)
                plan.gather_cfg(out, local)
                return out
    return _plain_forward(latents, cond, **fwd)


def _batch_rows(rows, name, rep, B, S0, dim, ws):
    """Token rows [S0 or B S0, dim] -> [B S0, dim]: one sample's rows are replicated into workspace buffer `rep`,
    rows of every sample are returned as they are (`name`: the input, for the shape error)."""
    if rows.dim() != 2 or rows.shape[1] != dim or rows.shape[0] not in (S0, B * S0):
        raise ValueError(f"model_fn_wan_video: {name} {tuple(rows.shape)} are not [{S0} or {B} * {S0}, {dim}]")
    if rows.shape[0] == B * S0:
        return rows
    return ws.get(rep, (B * S0, dim)).view(B, S0, dim).copy_(rows.view(1, S0, dim).expand(B, S0, dim)).view(B * S0, dim)


def _plain_forward(latents, cond, *, dit, vace, animate_adapter, timestep, context, vace_scale, sp, slg_blocks,
                   cfg_sample, tea_cache, seg):
    """The forward of one batch on this rank, every raw input of `cond` resolved here (a CFG-parallel rank
    computes only its own sample's reference tokens, pose rows and face K / V).

    seg (the first-frame segment): latent frame 0's n0 = (H/2)(W/2) tokens are modulated with timestep 0 and
    every other token with `timestep`.  The reference builds a per-token [1, S, 6, dim] modulation; it has two
    distinct rows, so here the time embedding runs on (0, bf16(timestep)) and every modulated LayerNorm and
    gated GEMM picks row (token >= n0) of its sample's two (RunCtx.seg_rows, include/vstyler_seg.h).

    y is read in place by the patch embedding, behind the latents' channels.  Of the embedded clip_feature the
    first 257 rows are the blocks' image keys, any further rows join the text keys (wan_video_dit.py:172-174).

    The reference tokens: dit.ref_conv turns reference_latents into n = (H/2)(W/2) tokens in front of every
    sample's S: the forward is the ordinary one over the grid (T + 1, H/2, W/2) whose frame 0 comes from
    ref_conv, and the head's rows n.. are unpatchified.  The camera adapter's output is added to the patch
    embedding's in that GEMM's epilogue.

    pose_latents: their patch embedding is added to the tokens of latent frames 1.. in the patch-embedding
    GEMM's epilogue (after_patch_embedding: bf16(x + bf16(pose))).  animate_face_motion: the face encoder turns
    the motion vectors into N motion tokens per latent frame behind a zero frame, and after every fifth block
    a FaceBlock cross-attends each frame's tokens to them (vs_face_attn)."""
    device = latents.device
    ws = _workspace(device)
    B, L = context.shape[0], context.shape[1]
    Tl, hw = latents.shape[2], (latents.shape[3] // 2) * (latents.shape[4] // 2)    # tokens per latent frame
    y, clip_feature, vace_context, animate_kv = cond.y, cond.clip_feature, cond.vace_context, cond.animate_kv
    use_face = cond.animate_face_motion is not None or animate_kv is not None
    # every CFG sample starts from the same rows when the latents, the timestep (and the VACE context)
    # are shared (the cfg_merge broadcast below): the first blocks' self-attention halves are then
    # computed once for all samples (DiTBlock shared_prefix)
    shared = B > 1 and latents.shape[0] == 1 and timestep.numel() == 1 and (y is None or y.shape[0] == 1)
    ref = cond.reference_tokens
    if ref is None and cond.reference_latents is not None:
        ref = dit.ref_tokens(cond.reference_latents, ws)
    if ref is not None:
        if ref.dim() != 2 or ref.shape[1] != dit.dim or ref.shape[0] not in (hw, B * hw):
            raise ValueError(f"model_fn_wan_video: reference_tokens {tuple(ref.shape)} are not [{hw} or "
                             f"{B} * {hw}, {dit.dim}]")
        shared = shared and ref.shape[0] == hw
    shared_vace = shared and vace_context is not None and vace_context.shape[0] == 1
    if y is not None:
        if y.shape[0] not in (1, B) or tuple(y.shape[2:]) != tuple(latents.shape[2:]):
            raise ValueError(f"model_fn_wan_video: y {tuple(y.shape)} does not match latents {tuple(latents.shape)} "
                             f"(batch 1 or {B})")
        y = y.to(device=device, dtype=BF16)
    if clip_feature is not None and clip_feature.shape[0] not in (1, B):
        raise ValueError(f"model_fn_wan_video: clip_feature batch {clip_feature.shape[0]} (1 or {B})")
    if latents.shape[0] != B and y is None:
        latents = latents.expand(B, *latents.shape[1:])
    latents = latents.to(BF16).contiguous()
    timestep = timestep.reshape(-1).to(device=device, dtype=BF16)
    if timestep.shape[0] != B:
        timestep = timestep.expand(B).contiguous()

    if seg:     # (0, bf16(t)) per sample: t [2 B, D], t_mod [2 B, 6, D], rows 2 b / 2 b + 1 = b's two segments
        timestep = torch.stack([torch.zeros_like(timestep), timestep], dim=1).reshape(-1)
    t, t_mod = dit.time_embed(timestep, ws)
    ctx = dit.text_embed(context.to(BF16), ws)
    extra = {}      # the patch embedding's keywords: none without conditioning
    cam = cond.camera_tokens    # (a loop hands the replicated rows: camera_token_rows(batch=B))
    if cam is None and cond.control_camera_latents_input is not None:
        cam = dit.control_adapter(cond.control_camera_latents_input)
    if cam is not None:
        extra["residual"] = _batch_rows(cam, "camera_tokens", "cam_rep", B, Tl * hw, dit.dim, ws)
    pose = cond.pose_tokens
    if pose is None and cond.pose_latents is not None:
        if tuple(cond.pose_latents.shape[3:]) != tuple(latents.shape[3:]):
            raise ValueError(f"model_fn_wan_video: pose_latents {tuple(cond.pose_latents.shape)} do not match "
                             f"latents {tuple(latents.shape)}")
        pose = animate_adapter.pose_rows(cond.pose_latents, Tl, ws)
    if pose is not None:
        extra["residual"] = _batch_rows(pose, "pose_tokens", "pose_rep", B, Tl * hw, dit.dim, ws)   # one pose for all
        if B > 1 and extra["residual"] is pose:
            shared = False                      # per-sample rows: block 0 sees different samples
    if use_face:
        if animate_kv is None:
            motion = cond.animate_face_motion
            if motion.dim() != 3 or motion.shape[0] not in (1, B):
                raise ValueError(f"model_fn_wan_video: animate_face_motion {tuple(motion.shape)}: expected "
                                 f"[1 or {B}, T_face, {animate_adapter.face_encoder.in_dim}]")
            animate_kv = animate_adapter.face_kv(animate_adapter.motion_tokens(motion, ws), ws)
        for kv in animate_kv:
            if kv.dim() != 3 or kv.shape[0] not in (1, B) or kv.shape[1] % Tl or not 1 <= kv.shape[1] // Tl <= 8 or \
                    kv.shape[2] != 2 * dit.dim:
                raise ValueError(f"model_fn_wan_video: the face motion covers {tuple(kv.shape)} key rows: expected "
                                 f"[1 or {B}, {Tl} latent frames * N (1..8), {2 * dit.dim}] (T_face frames give "
                                 f"((T_face - 1) // 2) // 2 + 2 latent frames)")
    if ref is not None:
        extra["skip"] = hw
    if y is not None:       # cat([latents, y], dim=1) read in place; batch-1 operands broadcast over the CFG batch
        extra.update(y=y, batch=B)
    x, grid = dit.patch_embedding(latents, ws, "x", **extra)
    S = grid[0] * grid[1] * grid[2]
    if ref is not None:
        # the reference tokens are frame 0 of a grid one frame longer (wan_video_new.py:1389-1390: concat in
        # front, RoPE for f + 1 frames): nothing below knows the difference
        K.ref_rows(ref, x, B, hw, S)
        grid, S = (grid[0] + 1, grid[1], grid[2]), hw + S
    img = None
    if clip_feature is not None:
        # context = cat([img_emb(clip_feature), text]) split as CrossAttention.forward does: the first
        # 257 rows are the image keys, the rest (the second image of a 514-row feature) text keys
        emb = dit.img_embed(clip_feature.to(device), ws)
        Bc, N, D = clip_feature.shape[0], clip_feature.shape[1], dit.dim
        emb = emb.view(Bc, N, D)
        img = emb[:, :IMG_TOKENS]
        if N > IMG_TOKENS:
            more = N - IMG_TOKENS
            img = ws.get("img_keys", (Bc, IMG_TOKENS, D))
            img.copy_(emb[:, :IMG_TOKENS])
            ctx2 = ws.get("ctx_img", (B, more + L, D))       # built once per forward
            ctx2[:, :more].copy_(emb[:, IMG_TOKENS:].expand(B, more, D))
            ctx2[:, more:].copy_(ctx.view(B, L, D))
            ctx, L = ctx2.view(B * (more + L), D), more + L
        img = img.reshape(Bc * IMG_TOKENS, D)

    if sp is not None and sp.world_size == 1 and not getattr(sp, "force_collectives", False):
        sp = None
    rc = RunCtx(B, S, grid, dit.rope(device), ctx, L, ws)
    if img is not None:
        rc.img, rc.img_batch = img, clip_feature.shape[0]
    if seg:
        rc.seg_rows = grid[1] * grid[2]     # the tokens of latent frame 0 (T == 1: every row)

    vace_x = None
    if vace_context is not None:
        vc = vace_context.to(BF16)
        if vc.shape[0] != B:
            vc = vc.expand(B, *vc.shape[1:])
        vace_x, _ = vace.vace_patch_embedding(vc.contiguous(), ws, "vace")

    # TeaCache (wan_video_new.py:1398-1402): decided on one prompt's t_mod before the blocks
    tea_skip = tea_cache.check(dit, x, t_mod[0:1]) if tea_cache is not None else False
    if sp is not None:
        x, vace_x, rc = sp.shard_tokens(x, vace_x, rc)

    if tea_skip:
        tea_cache.update(x)                                     # :1418-1419 (VACE not needed)
    else:
        if tea_cache is not None:
            tea_cache.begin(x)
        hints = vace(x, vace_x, t_mod, rc, shared_prefix=shared_vace) if vace_x is not None else None
        vmap = vace.vace_layers_mapping if hints is not None else {}
        for i, blk in enumerate(dit.blocks):
            # a batch-1 forward of CFG sample 1 (CFG-parallel rank) skips the slg blocks outright
            if B == 1 and cfg_sample == 1 and i in slg_blocks:
                continue
            hint = hints[vmap[i]] if i in vmap else None
            skip = B > 1 and i in slg_blocks
            blk(x, t_mod, rc, hint=hint, hint_scale=float(vace_scale), only_batch=0 if skip else None,
                shared_prefix=shared and i == 0)
            if use_face:                                        # after_transformer_block
                animate_adapter.after_block(i, x, animate_kv, rc)
        if tea_cache is not None:
            tea_cache.store(x)                                  # :1455-1456
    out = dit.head(x, t, rc)
    if sp is not None:
        out = sp.gather_tokens(out, rc)
    T, H2, W2 = grid
    if ref is not None:                                         # :1464-1465: drop the reference rows
        lat = torch.empty((B, dit.out_dim, T - 1, 2 * H2, 2 * W2), device=device, dtype=BF16)
        return K.unpatchify_skip(out, lat, hw)
    lat = torch.empty((B, dit.out_dim, T, 2 * H2, 2 * W2), device=device, dtype=BF16)
    return K.unpatchify(out, lat)
