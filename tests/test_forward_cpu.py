"""vstyler.forward without a GPU: the support matrix through both of its callers (model_fn_wan_video and the
pipeline's samplers), the record of what rides along a forward under its two splits, and the order of the checks.
Shapes: latents [1, 16, 3, 8, 12] (24 tokens per latent frame), dim 256, context [1, 8, 4096]; the models live on
the meta device, so nothing here can compute."""
import dataclasses
from dataclasses import dataclass

import pytest
import torch

import animate_util as A
import ti2v_util as T
from vstyler.forward import EXCLUDES

HW, FRAMES, DIM = 24, 3, 256
PAIRS = [(f, x) for f, row in EXCLUDES for x in row]


@pytest.fixture(scope="module")
def models():
    from vstyler.models import WanAnimateAdapter, WanModel
    cfg = A.tiny_cfg()
    dit = WanModel(dim=DIM, in_dim=36, ffn_dim=cfg["ffn_dim"], out_dim=16, text_dim=4096, freq_dim=256, eps=1e-6,
                   patch_size=(1, 2, 2), num_heads=2, num_layers=6, has_image_input=True, device="meta")
    ad = WanAnimateAdapter(dim=DIM, num_heads=2, num_layers=6, in_dim=32, device="meta")
    ti2v = T.build(T.TINY_TI2V, None, device="meta")
    assert ti2v.seperated_timestep and not dit.seperated_timestep
    return dit, ad, ti2v


def _lat():
    return torch.zeros(1, 16, FRAMES, 8, 12)


# ------------------------------------------------------------------------------------- 1. the support matrix
def _model_fn_feature(name, ad):
    """model_fn_wan_video's keywords that switch one feature on (None: it has no such argument)."""
    return {"animate": dict(animate_adapter=ad, pose_latents=torch.zeros(1, 16, 2, 8, 12)),
            "first_frame": dict(fuse_vae_embedding_in_latents=True),
            "windows": dict(sliding_window_size=2, sliding_window_stride=1),
            "tea_cache": dict(tea_cache=object()),
            "vace": dict(vace=object(), vace_context=torch.zeros(1, 96, FRAMES, 8, 12)),
            "reference": dict(reference_latents=torch.zeros(1, 16, 1, 8, 12)),
            "camera": dict(camera_tokens=torch.zeros(FRAMES * HW, DIM)),
            "slg": dict(slg_blocks=(1,)),
            "sp": dict(use_unified_sequence_parallel=True),
            "dit2": None}[name]


def _pipe_feature(pipe, name, dit, ad):
    """Switches one feature on for pipe.denoise: sets the pipeline's attribute or returns the keywords (None: denoise
    cannot express it)."""
    if name == "animate":
        pipe.animate_adapter = ad
        return dict(pose_latents=torch.zeros(1, 16, 2, 8, 12))
    if name == "vace":
        pipe.vace = object()
        return dict(vace_context=torch.zeros(1, 96, FRAMES, 8, 12))
    if name == "sp":
        pipe.use_unified_sequence_parallel = True
        return {}
    if name == "dit2":
        pipe.dit2 = dit
        return {}
    return {"first_frame": dict(first_frame_latents=torch.zeros(1, 16, 1, 8, 12)),
            "windows": dict(sliding_window_size=2, sliding_window_stride=1),
            "tea_cache": dict(tea_cache=object()),
            "reference": dict(reference_latents=torch.zeros(1, 16, 1, 8, 12)),
            "camera": dict(control_camera_latents_input=torch.zeros(1, 24, FRAMES, 64, 96)),
            "slg": None}[name]


@pytest.mark.parametrize("feature,excluded", PAIRS)
def test_every_excluded_pair_raises_through_both_callers(models, feature, excluded):
    from vstyler import WanVideoPipeline, model_fn_wan_video
    from vstyler.forward import FEATURES
    dit, ad, ti2v = models
    reached = 0
    a, b = _model_fn_feature(feature, ad), _model_fn_feature(excluded, ad)
    if a is not None and b is not None:
        # the first-frame segment is a property of the DiT; the animate path refuses the flag on any DiT
        model = ti2v if "first_frame" in (feature, excluded) and feature != "animate" else dit
        with pytest.raises(NotImplementedError) as e:
            model_fn_wan_video(model, latents=_lat(), timestep=torch.tensor([500.0]), context=torch.zeros(1, 8, 4096),
                               **a, **b)
        assert FEATURES[excluded] in str(e.value) and FEATURES[feature] in str(e.value)
        reached += 1
    pipe = WanVideoPipeline(device="cpu")
    pipe.dit = dit

    def no_forward(**kw):
        pytest.fail("the forward ran: the support matrix was not checked first")
    pipe.model_fn = no_forward
    a, b = _pipe_feature(pipe, feature, dit, ad), _pipe_feature(pipe, excluded, dit, ad)
    if a is not None and b is not None:
        ctx = torch.zeros(1, 8, 4096)
        with pytest.raises(NotImplementedError) as e:
            pipe.denoise(_lat(), ctx, ctx, num_inference_steps=2, **a, **b)
        assert FEATURES[excluded] in str(e.value) and FEATURES[feature] in str(e.value)
        reached += 1
    assert reached, "a pair of the table that no caller can express"


def test_table_is_the_issue_s_and_everything_else_is_allowed():
    from vstyler.forward import EXCLUDES, FEATURES, check_support
    assert dict(EXCLUDES) == {
        "animate": ("windows", "tea_cache", "dit2", "vace", "reference", "first_frame", "camera", "slg"),
        "first_frame": ("sp", "windows", "tea_cache", "vace", "dit2"),
        "windows": ("tea_cache", "camera"),
        "dit2": ("tea_cache",)}
    assert set(FEATURES) == {"animate", "first_frame", "windows", "tea_cache", "vace", "reference", "camera", "slg", "sp",
                             "dit2"}
    check_support({}, "test")
    check_support({f: False for f in FEATURES}, "test")
    names = sorted(FEATURES)
    allowed = 0
    for i, a in enumerate(names):
        check_support({a: True}, "test")
        for b in names[i + 1:]:
            if (a, b) in PAIRS or (b, a) in PAIRS:
                with pytest.raises(NotImplementedError, match="^test: "):
                    check_support({a: True, b: True}, "test")
            else:
                check_support({a: True, b: True}, "test")
                allowed += 1
    assert allowed == 45 - len(PAIRS)
    with pytest.raises(KeyError):
        check_support({"s2v": True}, "test")


# ---------------------------------------------------------------------------- 2. nothing rides a split unaccounted
def _per_sample(g):
    def r(*shape):
        return torch.randn(shape, generator=g)
    return dict(y=r(2, 20, FRAMES, 8, 12), y_windows=[r(2, 20, 2, 8, 12), r(2, 20, 2, 8, 12)], clip_feature=r(2, 257, 8),
                vace_context=r(2, 96, FRAMES, 8, 12), vace_context_windows=[r(2, 96, 2, 8, 12), r(2, 96, 2, 8, 12)],
                reference_latents=r(2, 16, 8, 12), reference_tokens=r(2 * HW, DIM),
                control_camera_latents_input=r(1, 24, FRAMES, 64, 96), camera_tokens=r(2 * FRAMES * HW, DIM),
                pose_latents=r(2, 16, 2, 8, 12), pose_tokens=r(2 * FRAMES * HW, DIM), animate_face_motion=r(2, 5, 32),
                animate_kv=[r(2, FRAMES * 5, 2 * DIM), r(2, FRAMES * 5, 2 * DIM)])


def _shared(g):
    def r(*shape):
        return torch.randn(shape, generator=g)
    return dict(y=r(1, 20, FRAMES, 8, 12), y_windows=[r(1, 20, 2, 8, 12), r(1, 20, 2, 8, 12)], clip_feature=r(1, 257, 8),
                vace_context=r(1, 96, FRAMES, 8, 12), vace_context_windows=[r(1, 96, 2, 8, 12), r(1, 96, 2, 8, 12)],
                reference_latents=r(1, 16, 8, 12), reference_tokens=r(HW, DIM),
                control_camera_latents_input=r(1, 24, FRAMES, 64, 96), camera_tokens=r(FRAMES * HW, DIM),
                pose_latents=r(1, 16, 2, 8, 12), pose_tokens=r(FRAMES * HW, DIM), animate_face_motion=r(1, 5, 32),
                animate_kv=[r(1, FRAMES * 5, 2 * DIM), r(1, FRAMES * 5, 2 * DIM)])


# what sample(c) of the per-sample form must be, field by field
SAMPLE_OF = {
    "y": lambda v, c: v[c:c + 1], "y_windows": lambda v, c: [x[c:c + 1] for x in v],
    "clip_feature": lambda v, c: v[c:c + 1], "vace_context": lambda v, c: v[c:c + 1],
    "vace_context_windows": lambda v, c: [x[c:c + 1] for x in v], "reference_latents": lambda v, c: v[c:c + 1],
    "reference_tokens": lambda v, c: v[c * HW:(c + 1) * HW], "control_camera_latents_input": lambda v, c: v,
    "camera_tokens": lambda v, c: v[c * FRAMES * HW:(c + 1) * FRAMES * HW], "pose_latents": lambda v, c: v[c:c + 1],
    "pose_tokens": lambda v, c: v[c * FRAMES * HW:(c + 1) * FRAMES * HW],
    "animate_face_motion": lambda v, c: v[c:c + 1], "animate_kv": lambda v, c: [x[c:c + 1] for x in v]}


def _same(got, want, identical=False):
    if isinstance(want, list):
        return isinstance(got, list) and len(got) == len(want) and all(_same(g, w, identical) for g, w in zip(got, want))
    return got is want if identical else got.shape == want.shape and torch.equal(got, want)


def test_sample_cuts_every_field_to_its_cfg_sample():
    from vstyler.forward import Conditioning
    full = _per_sample(torch.Generator().manual_seed(3))
    cond = Conditioning(**full)
    for c in (0, 1):
        mine = cond.sample(c, HW, FRAMES)
        for f in dataclasses.fields(Conditioning):
            assert f.name in SAMPLE_OF, f"no expectation for Conditioning.{f.name}"
            assert full[f.name] is not None
            assert _same(getattr(mine, f.name), SAMPLE_OF[f.name](full[f.name], c)), (f.name, c)
    assert cond.sample(1, HW, FRAMES).control_camera_latents_input is full["control_camera_latents_input"]
    # the two samples differ wherever a field has two
    a, b = cond.sample(0, HW, FRAMES), cond.sample(1, HW, FRAMES)
    assert not torch.equal(a.pose_tokens, b.pose_tokens) and not torch.equal(a.animate_kv[1], b.animate_kv[1])
    one = _shared(torch.Generator().manual_seed(4))
    mine = Conditioning(**one).sample(1, HW, FRAMES)
    for f in dataclasses.fields(Conditioning):
        assert _same(getattr(mine, f.name), one[f.name], identical=True), f.name
    empty = Conditioning().sample(1, HW, FRAMES)
    assert all(getattr(empty, f.name) is None for f in dataclasses.fields(Conditioning))


def test_window_cuts_y_and_the_vace_context_and_passes_the_rest(monkeypatch):
    from vstyler import kernels as K
    from vstyler.forward import Conditioning
    from vstyler.models import Workspace
    from vstyler.window import plan_windows
    calls = []

    def gather(src, t0, dst):
        calls.append((t0, dst.shape[2]))
        return dst.copy_(src[:, :, t0:t0 + dst.shape[2]])
    monkeypatch.setattr(K, "window_gather", gather)
    plan = plan_windows(FRAMES, 2, 1)
    assert plan.windows == [(0, 2), (1, 3)]
    full = _per_sample(torch.Generator().manual_seed(5))
    full = {k: (v.to(torch.bfloat16) if k in ("y", "vace_context") else v) for k, v in full.items()}
    cut = ("y", "vace_context")
    ws = Workspace("cpu")
    raw = Conditioning(**dict(full, y_windows=None, vace_context_windows=None))
    for i, (t, t_) in enumerate(plan.windows):
        w = raw.window(i, t, t_, ws)
        assert torch.equal(w.y, full["y"][:, :, t:t_]) and torch.equal(w.vace_context, full["vace_context"][:, :, t:t_])
        assert w.y.data_ptr() == ws.get("win_y", w.y.shape).data_ptr()
        assert w.vace_context.data_ptr() == ws.get("win_vace", w.vace_context.shape).data_ptr()
        assert w.y_windows is None and w.vace_context_windows is None
        for f in dataclasses.fields(Conditioning):
            assert f.name in cut or f.name.endswith("_windows") or getattr(w, f.name) is full[f.name], f.name
    assert calls == [(0, 2), (0, 2), (1, 2), (1, 2)]
    pre = Conditioning(**full)                              # the pre-cut lists win, picked by index: no gather
    for i, (t, t_) in enumerate(plan.windows):
        w = pre.window(i, t, t_, ws)
        assert w.y is full["y_windows"][i] and w.vace_context is full["vace_context_windows"][i]
        for f in dataclasses.fields(Conditioning):
            assert f.name in cut or getattr(w, f.name) is full[f.name], f.name
    assert len(calls) == 4
    none = Conditioning(clip_feature=full["clip_feature"]).window(0, 0, 2, ws)
    assert none.y is None and none.vace_context is None and none.clip_feature is full["clip_feature"]


def test_a_field_without_a_rule_is_an_error():
    from vstyler.forward import Conditioning
    from vstyler.models import Workspace

    @dataclass
    class More(Conditioning):
        audio_embeds: object = None
    more = More(audio_embeds=torch.zeros(2, 4))
    with pytest.raises(TypeError, match="audio_embeds"):
        more.sample(0, HW, FRAMES)
    with pytest.raises(TypeError, match="audio_embeds"):
        more.window(0, 0, 2, Workspace("cpu"))
    with pytest.raises(TypeError, match="audio_embeds"):     # even while it is unset
        More().sample(0, HW, FRAMES)


# --------------------------------------------------------------------------------------------- 3. the order
def test_first_pair_of_the_table_is_reported_and_window_arguments_come_first(models):
    from vstyler import model_fn_wan_video
    from vstyler.forward import FEATURES, check_support
    dit, ad, ti2v = models
    with pytest.raises(NotImplementedError) as e:
        check_support({"camera": True, "tea_cache": True, "windows": True, "animate": True}, "test")
    assert str(e.value) == f"test: {FEATURES['animate']} with {FEATURES['windows']} is not supported"
    base = dict(latents=_lat(), timestep=torch.tensor([500.0]), context=torch.zeros(1, 8, 4096))
    everything = dict(animate_adapter=ad, pose_latents=torch.zeros(1, 16, 2, 8, 12), tea_cache=object(),
                      camera_tokens=torch.zeros(FRAMES * HW, DIM))
    with pytest.raises(NotImplementedError) as e:
        model_fn_wan_video(dit, sliding_window_size=2, sliding_window_stride=1, **everything, **base)
    assert str(e.value) == f"model_fn_wan_video: {FEATURES['animate']} with {FEATURES['windows']} is not supported"
    # one window is not the feature: the next pair of the row
    with pytest.raises(NotImplementedError, match="tea_cache"):
        model_fn_wan_video(dit, sliding_window_size=3, sliding_window_stride=1, **everything, **base)
    for size, stride in ((2, 3), (2, None), (2.0, 1), (0, 0)):
        with pytest.raises(ValueError, match="sliding_window"):
            model_fn_wan_video(None, sliding_window_size=size, sliding_window_stride=stride, **everything, **base)
