"""CPU: the per-launch replay helper (tests/_sr_replay.py) proved before the GPU tests trust it.

(1) Self-check: the replay functions chained into a whole float64 training step (each launch's value stored as the next
    launch's operand) give the oracle's own output, intermediates and every autograd gradient back to 1e-10.
(2) Seeded defects: the chained state carries one defect at a time - in the STATE, as a wrong kernel or a wrong launch argument
    would leave it - and the per-launch check must fail first at the launch that was seeded, and nowhere on the clean state.
(3) The readers: Sl / CatBuf slices (interleaved and slice-planar) and the one-bit mask words."""
import copy

import pytest
import torch
import torch.nn.functional as F

import _sr_replay as R
from oracle import sr_oracle, synth

FLOW_GAIN = 20.0        # motion_estimator.flow_net.6 scaled: flows of a few pixels instead of 0.1 px (warp away from the identity)
Fc, NB, WIN, SCALE, B, H, W = 32, 2, 1, 2, 2, 12, 16
T = 2 * WIN + 1


def scaled_state(s, F_, nb, win):
    sd = synth.formula_state(3, s, F_, nb, win, gain=synth.GOLDEN_GAIN)
    for n in ("weight", "bias"):
        sd[f"motion_estimator.flow_net.6.{n}"] = sd[f"motion_estimator.flow_net.6.{n}"] * FLOW_GAIN
    return sd


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def chain(bn_on_the_fly, head_fused):
    sd = scaled_state(SCALE, Fc, NB, WIN)
    P = R.params64(sd)
    x = synth.formula_clip(B, T, H, W).double()
    tgt = synth.formula_target(B, H * SCALE, W * SCALE).double()
    S = R.new_state(x, Fc, NB, SCALE, bn_on_the_fly=bn_on_the_fly, head_fused=head_fused)
    R.walk_forward(S, P, R.ident, R.Builder(S))
    S["dout"] = 2.0 * (S["out"] - tgt) / tgt.numel()
    R.walk_backward(S, P, R.ident, R.Builder(S))
    return sd, P, x, tgt, S


@pytest.fixture(scope="module")
def clean():
    return chain(True, True)


@pytest.mark.parametrize("bn_on_the_fly,head_fused", [(True, True), (False, False)])
def test_chained_replay_is_the_oracle(bn_on_the_fly, head_fused):
    sd, P, x, tgt, S = chain(bn_on_the_fly, head_fused)
    ora = sr_oracle.OracleSR(3, SCALE, Fc, NB, WIN).double()
    ora.load_named(sd)
    ora.train()
    out, inter = ora(x, return_intermediate=True)
    F.mse_loss(out, tgt).backward()
    c, slots = S["meta"]["c"], S["meta"]["slots"]
    errs = {"out": rel(S["out"], out), "aggregated": rel(S["rdb.0.x"], inter["aggregated"]),
            "residual": rel(S[f"rdb.{NB}.x"], inter["residual"]), "fused": rel(S["fused"], inter["fused"])}
    for j, t in enumerate(slots):
        errs[f"features[{t}]"] = rel(S["features"][j * B:(j + 1) * B], inter["features"][t])
        errs[f"aligned[{t}]"] = rel(S["aligned"][:, t * Fc:(t + 1) * Fc], inter["aligned"][t])
        if t != c:
            errs[f"flow[{t}]"] = rel(S["flow.4"][(j - 1) * B:j * B], inter["flows"][t])
    named = ora.named()
    names = list(sr_oracle.param_shapes(3, SCALE, Fc, NB, WIN))
    for n in names:
        errs["grad:" + n] = rel(S["grad:" + n], named[n].grad)
    # the CBAM pieces of the helper are sr_oracle.cbam
    assert rel(S["rdb.0.x"], sr_oracle.cbam(P, S["weighted"])) < 1e-12
    worst = max(errs, key=errs.get)
    print(f"  chained replay vs oracle: worst {errs[worst]:.1e} ({worst}); flow max {S['flow.4'].abs().max():.2f} px")
    bad = {k: v for k, v in errs.items() if not v <= R.TOL_F64}
    assert not bad, bad
    assert S["flow.4"].abs().max() > 1.0, "the scaled flow layer should move the warp away from the identity"
    assert sorted(k[5:] for k in S if k.startswith("grad:")) == sorted(names)


def check(S, P):
    ck = R.Checker(S, False)
    R.walk_forward(S, P, R.ident, ck)
    R.walk_backward(S, P, R.ident, ck)
    return ck


def with_bits(S):
    """the chained state with its ReLU masks also as one-bit words, read back through the reader"""
    S = copy.deepcopy(S)
    for k in range(NB):
        for i in range(R.LAYERS):
            S[f"rdb.{k}.bits.{i}"] = R.read_bits(R.pack_bits(S[f"rdb.{k}.y.{i}"] > 0), R.GROWTH)
    S["a1bits"] = R.read_bits(R.pack_bits(S["a1"] > 0), Fc)
    for li in (1, 2, 3):
        S[f"flowbits.{li}"] = R.read_bits(R.pack_bits(S[f"flow.{li}"] > 0), R.FLOW_CH[li])
    return S


def test_clean_state_passes_every_launch(clean):
    sd, P, x, tgt, S = clean
    ck = check(with_bits(S), P)
    assert not ck.failures(), ck.report()
    # every parameter is claimed by exactly one replayed launch
    assert sorted(ck.claimed) == sorted(sr_oracle.param_shapes(3, SCALE, Fc, NB, WIN))
    launches = {r[0] for r in ck.rows}
    assert len(launches) > 40, sorted(launches)


def _flow_tap(S, P):
    w = P["motion_estimator.flow_net.2.weight"].clone()
    w[:, :, 0, 2] = 0
    S["flow.2"] = R.conv(S["flow.1"], w, P["motion_estimator.flow_net.2.bias"], R.ident, relu=True)


def _slice_off(S, P):
    cat = torch.cat([S["rdb.0.x"], S["rdb.0.y.0"]], 1)
    S["rdb.0.y.1"] = R.conv(torch.roll(cat, 1, 1), P["residual_blocks.0.layers.1.0.weight"],
                            P["residual_blocks.0.layers.1.0.bias"], R.ident, relu=True)


def _wgrad_row(S, P):
    dg = S["dg"].clone()
    dg[:, :, -1] = 0
    S["grad:gff.0.weight"] = R.conv_wgrad(S[f"rdb.{NB}.x"], dg, P["gff.0.weight"].shape, R.ident)[0]


def _alpha(S, P):
    cat = torch.cat([S["rdb.0.x"]] + [S[f"rdb.0.y.{i}"] for i in range(R.LAYERS)], 1)
    lff = R.conv(cat, P["residual_blocks.0.lff.weight"], P["residual_blocks.0.lff.bias"], R.ident)
    S["rdb.1.x"] = 0.25 * lff + S["rdb.0.x"]


def _mask_word(S, P):
    words = R.pack_bits(S["rdb.0.y.2"] > 0)
    shifted = words << 1
    n, y, x = (words != shifted).nonzero()[0].tolist()
    words[n, y, x] = shifted[n, y, x]
    S["rdb.0.bits.2"] = R.read_bits(words, R.GROWTH)


@pytest.mark.parametrize("seed,launch", [(_flow_tap, "flow.2"), (_slice_off, "rdb.0.layer.1"), (_wgrad_row, "gff.wgrad"),
                                         (_alpha, "rdb.0.lff"), (_mask_word, "rdb.0.layer.2")],
                         ids=["flow_tap_zeroed", "slice_one_channel_off", "wgrad_last_row_missing", "alpha_0.25", "mask_word_shifted"])
def test_seeded_defect_fails_at_its_launch(clean, seed, launch):
    sd, P, x, tgt, S = clean
    S = with_bits(S)
    seed(S, P)
    fails = check(S, P).failures()
    assert fails, f"the defect behind {launch} went unnoticed"
    assert fails[0][0] == launch, [f[:3] for f in fails]


# ------------------------------------------------------------------ readers
def test_bits_roundtrip_and_layout():
    g = torch.Generator().manual_seed(3)
    for C in (32, 64, 128):
        m = torch.rand(2, C, 5, 7, generator=g) > 0.5
        m[0, 31, 0, 0], m[0, C - 1, 1, 1] = True, True        # the sign bit of a word
        w = R.pack_bits(m)
        assert w.dtype == torch.int32 and tuple(w.shape) == ((2, 5, 7) if C == 32 else (2, 5, 7, C // 32))
        assert torch.equal(R.read_bits(w, C), m)
    # bit c % 32 of word c / 32 is channel c
    w = torch.zeros(1, 1, 1, 2, dtype=torch.int32)
    w[0, 0, 0, 1] = 1 << 3
    assert R.read_bits(w, 64)[0, :, 0, 0].nonzero().flatten().tolist() == [35]


@pytest.mark.parametrize("planar", [False, True])
def test_catbuf_readers(planar):
    from nerve_cl._nvq import CatBuf, Sl
    N, Hh, Ww, F_ = 2, 3, 5, 64
    dt = torch.bfloat16 if planar else torch.float32
    cat = CatBuf("cpu", N, Hh, Ww, F_, R.LAYERS, 256, dt, planar)
    ref = torch.arange(N * (F_ + 160) * Hh * Ww, dtype=torch.float32).reshape(N, F_ + 160, Hh, Ww) % 251
    nhwc = ref.permute(0, 2, 3, 1)
    cat.x().t[..., :F_] = nhwc[..., :F_].to(dt)
    for j in range(R.LAYERS):
        y = cat.y(j)
        y.t[..., y.coff:y.coff + 32] = nhwc[..., F_ + 32 * j:F_ + 32 * (j + 1)].to(dt)
    for cin in (F_, F_ + 32, F_ + 160):
        assert torch.equal(R.read_sl(cat.inp(cin)), ref[:, :cin].double())
    assert torch.equal(R.read_sl(cat.y(3)), ref[:, F_ + 96:F_ + 128].double())
    t = torch.arange(2 * 3 * 4 * 12, dtype=torch.float32).reshape(2, 3, 4, 12)
    assert torch.equal(R.read_sl(Sl(t, 4, 8)), t[..., 8:12].permute(0, 3, 1, 2).double())
    assert torch.equal(R.read_amax(torch.tensor([[3]], dtype=torch.int32)), torch.tensor([[3]]))
