"""CPU: the launch schedule of nerve_cl._engine, compared with traces recorded before the schedule was split into stage
functions.  tests/engine_schedule/digests.txt holds, for every case, the number of launches, the number of trace lines and the
SHA-256 of the whole trace (names, order and normalised arguments: one changed character changes it); its first line names the
commit it was recorded from.  One trace per distinct branch family is also committed in full (FULL: the SR net with the fused
bf16 extractor, plain and synchronised, with the unfused synchronised fp32 extractor, with the fp32 feature gradient and every
intermediate's gradient injected, with the unfused pointwise backward in bf16, and the light net in both modes), so that a
difference there is reported call by call and the schedule can be read; for any other case `--dump DIR` at both commits writes
the full traces to compare.

The recorder puts a proxy in the place of the `K` module inside _engine: every function _engine reaches through `K.` is
logged with its arguments in a normalised form before it runs, and so are _engine._allreduce_sum_ and every DEBUG_CAPTURE
key.  The arguments are bound to the wrapper's signature first: a parameter without a default is logged by position, any
other as name=value unless it has its default value (so `f(x)` and `f(x, bn=None)` are one operand list, as they are for the
kernel).  A tensor is logged as (ordinal of its storage by first appearance, shape, dtype, storage offset) where that view first
appears, `v<n>=...`, and as `v<n>` after that; an Sl as its tensor plus c / coff / plane, lists, tuples and scalars recursively;
conv_wgrad's `defer` queue as its length (its jobs are the conv_wgrad lines since the last wgrad_reduce_batch, which logs
them all).  The real _nvq wrappers still run on CPU tensors (their
shape checks and allocations are part of the schedule); what they would launch goes to a fake library whose entry points
return 0 (the few size queries return a value), and require_device / stream are inert.  No wrapper needed the device, so none
is stubbed.  A call that never reaches the library (pad4, bn_counts, new_bn_stats, dwconv_bn_fusable, a batch of no jobs:
host arithmetic and views) launches nothing and is left out: where it runs between two launches is not part of the
schedule, and the tensors it makes appear as operands of the launches.  Classes (K.CatBuf) and constants pass through the
proxy unlogged.

`python tests/test_engine_schedule_cpu.py --write COMMIT` records digests.txt and the full traces from the checked-out tree,
`--dump DIR` writes every case's full trace into DIR."""
import contextlib
import ctypes
import hashlib
import inspect
import os
import re
import sys
import types

import pytest
import torch

from nerve_cl import _engine, _nvq
from nerve_cl.models import LightweightSuperResolution, SuperResolutionNet

TRACES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "engine_schedule")
F, NB, H, W, B, SCALE = 64, 2, 16, 16, 1, 2
SWITCHES = ("NVQ_FUSED_PW_BWD", "NVQ_FUSED_DW_BWD", "NVQ_FUSED_BN_SUMS", "NVQ_PW_RECOMPUTE", "NVQ_BF16_FEATURE_GRAD",
            "NVQ_FUSED_DWPW", "NVQ_FUSED_TAIL", "NVQ_BF16_FEATURES", "NVQ_RELU_BITS", "NVQ_BF16_CBAM", "NVQ_PLANAR",
            "NVQ_FUSE_TAIL")
DTYPES = {torch.float32: "f32", torch.bfloat16: "bf16", torch.int32: "i32", torch.uint8: "u8", torch.float64: "f64",
          torch.int64: "i64"}


# ----------------------------------------------------------------------------- recorder
class FakeLib:
    """libnvq's entry points: 0 (success) for every launch, a value for the size queries the wrappers allocate from"""
    SIZES = {
        "nvq_wgrad_workspace_bytes": lambda: 1 << 20,
        "nvq_conv_pack_floats": lambda keep, cin_store, k, math: keep * cin_store * k * k,
        "nvq_rdb_backward_weights_floats": lambda f: sum(32 * (f + 32 * t) * 9 for t in range(5)) + f * (f + 160) * 9,
        "nvq_warp_backward_workspace_bytes": lambda n, h, w, mode: 4096,
        "nvq_tsum_blocks": lambda h, w: 2,
        "nvq_last_error": lambda: b"",
    }

    def __init__(self):
        self.launches = self.calls = 0

    def __getattr__(self, name):
        assert name in _nvq.SIGNATURES, name
        size = self.SIZES.get(name)

        def entry(*args):
            assert len(args) == len(_nvq.SIGNATURES[name][1]), name
            self.calls += 1
            if size is not None:
                return size(*args)
            self.launches += 1
            return 0
        return entry


class Recorder:
    def __init__(self, fake):
        self.fake, self.lines, self.ords, self.views, self.alive = fake, [], {}, {}, []

    def norm(self, a):
        if torch.is_tensor(a):
            st = a.untyped_storage()
            key = st.data_ptr() if st.nbytes() else ("empty", id(st))
            if key not in self.ords:
                self.ords[key] = len(self.ords)
                self.alive.append(st)           # (a freed storage's address could come back under another tensor)
            text = "t%d[%s]%s@%d%s" % (self.ords[key], ",".join(map(str, a.shape)), DTYPES[a.dtype], a.storage_offset(),
                                       "" if a.is_contiguous() else "s%s" % list(a.stride()))
            if text in self.views:
                return "v%d" % self.views[text]
            self.views[text] = len(self.views)
            return "v%d=%s" % (self.views[text], text)
        if isinstance(a, _nvq.Sl):
            return "Sl(%s c%d+%d p%d)" % (self.norm(a.t), a.c, a.coff, a.plane)
        if isinstance(a, (list, tuple)):
            body = ",".join(self.norm(x) for x in a)
            return "[%s]" % body if isinstance(a, list) else "(%s)" % body
        if isinstance(a, ctypes.Structure):
            return type(a).__name__
        assert a is None or isinstance(a, (bool, int, float, str, torch.dtype, torch.device)), type(a)
        return repr(a)

    def call(self, name, sig, args, kwargs):
        bound = sig.bind(*args, **kwargs)
        parts = []
        for pname, v in bound.arguments.items():
            default = sig.parameters[pname].default
            if default is inspect.Parameter.empty:
                parts.append(self.norm(v))
            elif pname == "defer" and v is not None:
                parts.append("defer=%d" % len(v))       # (the queue so far: each job is the conv_wgrad line that appended it)
            elif not (v is default or (type(v) is type(default) and not torch.is_tensor(v) and v == default)):
                parts.append("%s=%s" % (pname, self.norm(v)))
        self.lines.append("%s(%s)" % (name, ", ".join(parts)))

    def wrap(self, name, fn):
        sig = inspect.signature(fn)

        def logged(*args, **kwargs):
            at, known, seen, calls = len(self.lines), len(self.ords), len(self.views), self.fake.calls
            self.call(name, sig, args, kwargs)
            out = fn(*args, **kwargs)
            if self.fake.calls == calls:        # nothing reached the library: not part of the schedule
                del self.lines[at]
                self.ords = {k: v for k, v in self.ords.items() if v < known}
                self.views = {k: v for k, v in self.views.items() if v < seen}
                del self.alive[known:]
            return out
        return logged


class KProxy:
    """`K` as _engine sees it: functions logged, everything else (and every assignment, K.TIMER_TAG) the real module's"""

    def __init__(self, rec):
        object.__setattr__(self, "_rec", rec)

    def __getattr__(self, name):
        v = getattr(_nvq, name)
        return self._rec.wrap(name, v) if isinstance(v, types.FunctionType) else v

    def __setattr__(self, name, value):
        setattr(_nvq, name, value)


class CaptureLog(dict):
    def __init__(self, rec):
        super().__init__()
        self.rec = rec

    def __setitem__(self, key, value):
        self.rec.lines.append("capture:%s" % key)
        super().__setitem__(key, value)


@contextlib.contextmanager
def host_engine(rec, fake, env, small):
    """_engine on the host: the proxy and the fake library in place, the A/B switches at their defaults except `env`"""
    saved_env = {k: os.environ.get(k) for k in SWITCHES}
    saved = [(m, n, getattr(m, n)) for m, n in (
        (_nvq, "lib"), (_nvq, "stream"), (_nvq, "require_device"), (_nvq, "TIMER"), (_nvq, "TIMER_TAG"), (_engine, "K"),
        (_engine, "_allreduce_sum_"), (_engine, "DEBUG_CAPTURE"), (_engine, "SMALL_STEP_PIXELS"), (_engine, "_TAIL_ROWS"),
        (_engine, "_ws_cache"), (_engine, "_ws_multi_cache"))]
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        _nvq.lib, _nvq.stream, _nvq.require_device = (lambda: fake), (lambda: None), (lambda *a, **k: None)
        _nvq.TIMER, _nvq.TIMER_TAG = None, ""
        _engine.K = KProxy(rec)
        _engine._allreduce_sum_ = lambda t, group: rec.lines.append("_allreduce_sum_(%s, %s)" % (rec.norm(t), rec.norm(group)))
        _engine.DEBUG_CAPTURE = CaptureLog(rec)
        _engine.SMALL_STEP_PIXELS = 16 * 128 * 128 if small else 0
        _engine._TAIL_ROWS = 0
        _engine._ws_cache, _engine._ws_multi_cache = {}, {}
        yield
    finally:
        for m, n, v in saved:
            setattr(m, n, v)
        for k, v in saved_env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ----------------------------------------------------------------------------- cases
def _sr_need(plan, T):
    names = [n for _, ns in _engine.sr_stages(NB, T) for n in ns]
    pick = {
        "all": lambda n: True,
        "p2": lambda n: not n.startswith(("feature_extractor.", "motion_estimator.")),
        "p3": lambda n: n.startswith(("gff.", "upsampler.")),
        "p4": lambda n: False,                                                  # all frozen, the frames need a gradient
        "p5": lambda n: not n.startswith("residual_blocks."),
        "p6": lambda n: not re.match(r"feature_extractor\.body\.\d\.bn\.", n),
        "motion_frozen": lambda n: not n.startswith("motion_estimator."),
        "flow46_only": lambda n: n.startswith(("motion_estimator.flow_net.4", "motion_estimator.flow_net.6")),
        # further exits of the code that moved: a stage that runs for one weight gradient and needs no input gradient
        "body1_pw_only": lambda n: n == "feature_extractor.body.1.pointwise.weight",
        "body0_pw_only": lambda n: n == "feature_extractor.body.0.pointwise.weight",
        "head_bias_only": lambda n: n == "feature_extractor.head.0.bias",
        "cbam_sa_only": lambda n: n == "temporal_aggregator.refine.spatial_attention.conv.weight",
        "cbam_fc0_only": lambda n: n == "temporal_aggregator.refine.channel_attention.fc.0.weight",
        "rdb0_l2_only": lambda n: n == "residual_blocks.0.layers.2.0.weight",
    }[plan]
    return [n for n in names if pick(n)]


def _case(T=3, mode="bf16", small=True, training=True, deterministic=False, dframes=False, dinter=None, plan="all", env=None,
          sync=False, cached=False):
    return dict(T=T, mode=mode, small=small, training=training, deterministic=deterministic, dframes=dframes, dinter=dinter,
                plan=plan, env=env or {}, sync=sync, cached=cached)


SR_CASES = {}
for _m in ("bf16", "f32"):
    SR_CASES.update({
        f"{_m}_T3": _case(mode=_m), f"{_m}_T1": _case(T=1, mode=_m), f"{_m}_T3_large": _case(mode=_m, small=False),
        f"{_m}_T3_eval": _case(mode=_m, training=False), f"{_m}_T3_deterministic": _case(mode=_m, deterministic=True),
        f"{_m}_T3_dframes": _case(mode=_m, dframes=True), f"{_m}_T3_dinter_all": _case(mode=_m, dinter="all"),
        f"{_m}_T3_dinter_aggregated": _case(mode=_m, dinter="aggregated"), f"{_m}_T3_sync": _case(mode=_m, sync=True)})
    for _p in ("p2", "p3", "p4", "p5", "p6", "motion_frozen", "flow46_only", "body1_pw_only", "body0_pw_only", "head_bias_only"):
        SR_CASES[f"{_m}_T3_{_p}"] = _case(mode=_m, plan=_p, dframes=_p == "p4")
for _p in ("cbam_sa_only", "cbam_fc0_only", "rdb0_l2_only"):
    SR_CASES[f"bf16_T3_{_p}"] = _case(plan=_p)
for _e in ("NVQ_FUSED_PW_BWD=0", "NVQ_FUSED_DW_BWD=0", "NVQ_FUSED_BN_SUMS=1", "NVQ_PW_RECOMPUTE=0", "NVQ_BF16_FEATURE_GRAD=0",
           "NVQ_FUSED_DWPW=0", "NVQ_FUSED_TAIL=0"):
    SR_CASES["bf16_T3_" + _e.replace("=", "")] = _case(env=dict([_e.split("=")]))
SR_CASES["f32_T3_cached_features"] = _case(mode="f32", training=False, cached=True)

LIGHT_CASES = {}
for _m in ("bf16", "f32"):
    LIGHT_CASES.update({f"{_m}_train": _case(mode=_m), f"{_m}_eval": _case(mode=_m, training=False),
                        f"{_m}_sync": _case(mode=_m, sync=True)})
LIGHT_CASES.update({"f32_up_only": _case(mode="f32", plan="up_only"), "f32_head_only": _case(mode="f32", plan="head_only"),
                    "f32_frozen_depthwise": _case(mode="f32", plan="frozen_depthwise"),
                    "f32_block0_pw_only": _case(mode="f32", plan="block0_pw_only"), "f32_dframes": _case(mode="f32", dframes=True),
                    "f32_frozen_dframes": _case(mode="f32", plan="none", dframes=True)})


def _light_need(plan):
    names = [n for _, ns in _engine.light_stages() for n in ns]
    pick = {"all": lambda n: True, "none": lambda n: False, "up_only": lambda n: n == "net.6.weight",
            "head_only": lambda n: n.startswith("net.0."), "frozen_depthwise": lambda n: "depthwise" not in n,
            "block0_pw_only": lambda n: n == "net.2.pointwise.weight"}[plan]
    return [n for n in names if pick(n)]


def _modes(mode):
    return (_nvq.MATH_BF16, torch.bfloat16) if mode == "bf16" else (_nvq.MATH_F32, torch.float32)


def _finish(rec, fake, P):
    tracked = [int(P[n]) for n in sorted(P) if n.endswith("num_batches_tracked")]
    return "\n".join(["launches: %d" % fake.launches] + rec.lines + ["num_batches_tracked: %s" % tracked]) + "\n"


def record_sr(case) -> str:
    T = case["T"]
    math, act = _modes(case["mode"])
    torch.manual_seed(0)
    net = SuperResolutionNet(3, SCALE, F, NB, T // 2)
    P = net._tensor_dict()
    frames = torch.zeros(B, T, 3, H, W)
    fake = FakeLib()
    rec = Recorder(fake)
    with host_engine(rec, fake, case["env"], case["small"]):
        sync = {f"feature_extractor.body.{k}.bn": "group" for k in range(3)} if case["sync"] else None
        if case["cached"]:
            feats = _engine.extract_features(P, torch.zeros(B, T + 1, 3, H, W), F, math, act)
            _engine.forward(P, frames, F, NB, SCALE, False, math, act, features=feats[:T].contiguous())
            return _finish(rec, fake, P)
        out, sv = _engine.forward(P, frames, F, NB, SCALE, case["training"], math, act, sync=sync)
        rec.lines.append("-- backward")
        dinter = None
        if case["dinter"]:
            inter = _engine.intermediates(sv)
            dinter = [torch.zeros_like(t) if (case["dinter"] == "all" or i == 2 * T) else None for i, t in enumerate(inter)]
        need = _sr_need(case["plan"], T)
        G = {n: torch.empty_like(P[n]) for n in need}
        dframes = torch.empty_like(frames) if case["dframes"] else None
        plan = None if case["plan"] == "all" else _engine.backward_plan(need, case["dframes"], NB, T)
        _engine.backward(P, sv, torch.zeros_like(out), G, deterministic=case["deterministic"], dframes=dframes, plan=plan,
                         dinter=dinter)
    return _finish(rec, fake, P)


def record_light(case) -> str:
    math, act = _modes(case["mode"])
    torch.manual_seed(0)
    net = LightweightSuperResolution(SCALE)
    P = net._tensor_dict()
    x = torch.zeros(B, 3, H, W)
    fake = FakeLib()
    rec = Recorder(fake)
    with host_engine(rec, fake, case["env"], case["small"]):
        sync = {f"net.{k}.bn": "group" for k in _engine.LIGHT_BLOCKS} if case["sync"] else None
        out, sv = _engine.light_forward(P, x, SCALE, case["training"], math, act, sync=sync)
        rec.lines.append("-- backward")
        need = _light_need(case["plan"])
        G = {n: torch.empty_like(P[n]) for n in need}
        dframes = torch.empty(B, 1, 3, H, W) if case["dframes"] else None
        plan = None if case["plan"] == "all" else _engine.light_backward_plan(need, case["dframes"])
        _engine.light_backward(P, sv, torch.zeros_like(out), G, dframes=dframes, plan=plan)
    return _finish(rec, fake, P)


CASES = [("sr", n, record_sr, c) for n, c in SR_CASES.items()] + [("light", n, record_light, c) for n, c in LIGHT_CASES.items()]


FULL = ("sr-bf16_T3", "sr-bf16_T3_sync", "sr-f32_T3_sync", "sr-f32_T3_dinter_all", "sr-bf16_T3_NVQ_FUSED_PW_BWD0",
        "light-f32_sync", "light-bf16_train")


def _digest_line(case_id, text):
    lines = text.splitlines()
    return "%s %s %d %s" % (case_id, lines[0].split()[1], len(lines), hashlib.sha256(text.encode()).hexdigest())


def _recorded():
    with open(os.path.join(TRACES, "digests.txt")) as f:
        return {ln.split()[0]: ln.strip() for ln in f.read().splitlines()[1:]}


@pytest.mark.parametrize("net,name,record,case", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_schedule_is_the_recorded_one(net, name, record, case):
    case_id, got = f"{net}-{name}", record(case)
    if case_id in FULL:
        with open(os.path.join(TRACES, case_id + ".txt")) as f:
            want = f.read().splitlines()[1:]                # (line 0: the commit the trace was recorded from)
        for i, (g, w) in enumerate(zip(got.splitlines(), want)):
            assert g == w, f"{case_id}: line {i} differs\n  now:      {g}\n  recorded: {w}"
    assert _digest_line(case_id, got) == _recorded()[case_id], \
        f"{case_id}: (case, launches, lines, sha256) differ; compare the output of --dump at both commits"


def test_every_recorded_trace_has_a_case():
    assert sorted(_recorded()) == sorted(f"{c[0]}-{c[1]}" for c in CASES)
    assert sorted(os.listdir(TRACES)) == sorted(["digests.txt"] + [c + ".txt" for c in FULL])


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] in ("--write", "--dump"), "usage: --write COMMIT | --dump DIR"
    texts = {f"{c[0]}-{c[1]}": c[2](c[3]) for c in CASES}
    note = f"# recorded from commit {sys.argv[2]}\n"
    if sys.argv[1] == "--write":
        with open(os.path.join(TRACES, "digests.txt"), "w") as f_:
            f_.write(note + "".join(_digest_line(c, t) + "\n" for c, t in texts.items()))
    for c_, t_ in texts.items():
        if sys.argv[1] == "--dump" or c_ in FULL:
            with open(os.path.join(TRACES if sys.argv[1] == "--write" else sys.argv[2], c_ + ".txt"), "w") as f_:
                f_.write(note + t_)
