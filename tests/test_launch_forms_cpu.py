"""CPU: a mirror of the host rules that pick a kernel form from the size of the launch (conv_forward's `gs` loop,
conv_wgrad's pixel split, the persistent tile loops of the stem and depthwise weight gradients, conv_forward_bf16's
`underfilled` rule), with every constant read from the sources, and the one table of shapes that tests/test_launch_forms_gpu.py
runs.  Each row names the form it is meant to reach; the test here recomputes the rule for the row and fails when the shape
sits on the other side - so a changed threshold, or an edited shape, cannot move a GPU case off its form unnoticed."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "continual-learning-for-dynamic-video-quality-enhancement_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _ints(name, pattern, count=1):
    """the integer groups of every match of `pattern` in csrc/<name>; exactly `count` matches or a failure that says so"""
    found = [m.groups() for m in re.finditer(pattern, _src(name))]
    if len(found) != count:
        pytest.fail(f"csrc/{name}: expected {count} match(es) of /{pattern}/, found {len(found)} - the host rule this test "
                    f"mirrors has changed; update tests/test_launch_forms_cpu.py and the shapes of its table with it")
    return [tuple(int(v) for v in groups) for groups in found]


def _const(name, ident):
    return _ints(name, r"constexpr int(?: [A-Z_0-9]+ = \d+,)* " + ident + r" = (\d+)\b")[0][0]


def host_constants():
    c = {k: _const("conv_common.h", k) for k in ("TH", "TW", "WG_C", "WGRAD_MAX_WG", "NVQ_SMALL_IMAGE_TILES")}
    c["KC"] = _const("conv_igemm.hip", "KC")
    c["WR_Q"] = _const("conv_igemm.hip", "WR_Q")
    # choose_nt(): 16 / 32 / 64 output channels per packed slab
    _ints("conv_common.h", r"return cout <= 16 \? 16 : \(cout <= 32 \? 32 : 64\);")
    # while (gs * 2 <= NT / 16 && (long)grid.x * grid.y * gs * 2 <= 512) gs *= 2;
    c["GS_WG"] = _ints("conv_igemm.hip", r"while \(gs \* 2 <= NT / 16 && \(long\)grid\.x \* grid\.y \* gs \* 2 <= (\d+)\) gs \*= 2;")[0][0]
    # the form each (NT, gs) launches
    _ints("conv_igemm.hip", r"if \(gs == 1\) NVQ_LAUNCH_CONV\(2, KS, 1\);\s*\\\s*else NVQ_LAUNCH_CONV\(1, KS, 2\);")
    _ints("conv_igemm.hip", r"if \(gs == 1\) NVQ_LAUNCH_CONV\(4, KS, 1\);\s*\\\s*else if \(gs == 2\) NVQ_LAUNCH_CONV\(2, KS, 2\);"
                            r"\s*\\\s*else NVQ_LAUNCH_CONV\(1, KS, 4\);")
    # nsplit = WGRAD_MAX_WG / (nci * nco), at most ntiles, rounded down to a multiple of 8
    _ints("conv_igemm.hip", r"int nsplit = WGRAD_MAX_WG / \(nci \* nco\);")
    _ints("conv_igemm.hip", r"if \(nsplit > ntiles\) nsplit = ntiles;")
    _ints("conv_igemm.hip", r"if \(nsplit >= 8\) nsplit &= ~7;")
    # the reduce's four-chain loop and the lane loop of reduce_partials_kernel
    _ints("conv_igemm.hip", r"for \(; k \+ 3 \* WR_Q < nsplit; k \+= 4 \* WR_Q\)")
    _ints("conv_igemm.hip", r"for \(int b = lane; b < nblk; b \+= 64\)")
    a, b = _ints("fr_ops.hip", r"const int nblk = nt < (\d+) \? \(int\)nt : (\d+);")[0]
    assert a == b
    c["STEM_WG"] = a
    c["ST_T"] = _const("fr_ops.hip", "ST_T")
    _ints("fr_ops.hip", r"for \(int co0 = 0; co0 < Co; co0 \+= 64\)", 2)      # forward kernel and weight-gradient launcher
    caps = _ints("pointwise.hip", r"const int nb = ntiles < (\d+) \? ntiles : (\d+);", 2)     # bf16 full-line and fp32 tiled forms
    assert len({v for pair in caps for v in pair}) == 1
    c["DW_WG"] = caps[0][0]
    c["DT_H"], c["DT_W"], c["DT_C"] = (_const("pointwise.hip", k) for k in ("DT_H", "DT_W", "DT_C"))
    c["DB_C"] = _const("pointwise.hip", "DB_C")
    # conv_forward_bf16: the rule looks at one image's 16x32 tiles; the 32x32x16 form is automatic up to 128 input channels
    _ints("conv_bf16.hip", r"const bool underfilled = tilesX \* \(\(d\.h \+ 2 \* TH - 1\) / \(2 \* TH\)\) < NVQ_SMALL_IMAGE_TILES;")
    _ints("conv_bf16.hip", r"const int rows = d\.tile_rows == 0 && underfilled \? 8 : d\.tile_rows;")
    c["M32_CIN"] = _ints("conv_bf16.hip", r"\(rows == 162 \|\| rows == 164 \|\| \(rows == 0 && d\.cin <= (\d+)\)\)\)")[0][0]
    return c


def cdiv(a, b):
    return (a + b - 1) // b


def pad4(c):
    return (c + 3) // 4 * 4


# ----------------------------------------------------------------------------- the rules
def conv_f32_rule(c, cout, ks, N, H, W, cout_store=None):
    """nvq_conv_forward, fp32 math -> dict(g, gs, form = (NB, KS, GS) of conv_f32_kernel)"""
    NT = 16 if cout <= 16 else (32 if cout <= 32 else 64)
    ncz = cdiv(cout_store or pad4(cout), NT)
    g = cdiv(W, c["TW"]) * cdiv(H, c["TH"]) * N * ncz
    gs = 1
    while gs * 2 <= NT // 16 and g * gs * 2 <= c["GS_WG"]:
        gs *= 2
    return dict(g=g, gs=gs, form=(NT // 16 // gs, ks, gs))


def wgrad_f32_rule(c, cin_w, cout, N, H, W):
    """fp32 nvq_conv_wgrad -> dict(nsplit, tiles = (fewest, most) tiles a split walks, chains = the reduce's unrolled loop runs,
    bias_trips = trips of the bias blocks' lane loop)"""
    nci, nco = cdiv(cin_w, c["WG_C"]), cdiv(cout, c["WG_C"])
    ntiles = cdiv(W, c["TW"]) * cdiv(H, c["TH"]) * N
    nsplit = max(1, c["WGRAD_MAX_WG"] // (nci * nco))
    nsplit = min(nsplit, ntiles)
    if nsplit >= 8:
        nsplit &= ~7
    return dict(nsplit=nsplit, ntiles=ntiles, tiles=(ntiles // nsplit, cdiv(ntiles, nsplit)),
                chains=nsplit >= 4 * c["WR_Q"], bias_trips=cdiv(nsplit, 64))


def stem_rule(c, Co, N, H, W):
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    nt = N * cdiv(OH, c["ST_T"]) * cdiv(OW, c["ST_T"])
    wg = min(nt, c["STEM_WG"])
    return dict(tiles=nt, wg=wg, two_tiles=nt - wg if nt <= 2 * wg else None, per_wg=cdiv(nt, wg), reduce_trips=cdiv(wg, 64),
                passes=cdiv(Co, 64), live_last=Co - 64 * (cdiv(Co, 64) - 1))


def dw_rule(c, C, N, H, W, bf16):
    nt = N * cdiv(H, c["DT_H"]) * cdiv(W, c["DT_W"])
    wg = min(nt, c["DW_WG"])
    form = "bf16_full_line" if (C % c["DB_C"] == 0 and bf16) else ("tiled" if C % c["DT_C"] == 0 else "flat")
    return dict(tiles=nt, wg=wg, per_wg=cdiv(nt, wg), form=form, reduce_trips=cdiv(wg, 64))


def bf16_auto_rule(c, cin, cout, H, W):
    """conv_forward_bf16, 3x3, bf16 input, vector epilogue, tile_rows = 0 -> (underfilled, the tile_rows value that forces the
    form the automatic choice takes)"""
    assert 16 < cout <= 32 and H >= 2 * c["TH"]
    tiles16 = cdiv(W, c["TW"]) * cdiv(H, 2 * c["TH"])
    under = tiles16 < c["NVQ_SMALL_IMAGE_TILES"]
    return dict(tiles16=tiles16, underfilled=under, same_as=8 if under else (162 if cin <= c["M32_CIN"] else 16))


# ----------------------------------------------------------------------------- the table
FH, FW = 67, 97          # 9 tile rows (the last of 3 rows) x 4 tile columns (the last of 1 column): 36 ragged tiles per image
CIN = 40                 # two whole K chunks of 16 and a third of 8

CASES = []


def _case(name, kind, want, **shape):
    CASES.append(dict(name=name, kind=kind, want=want, **shape))


for _ks in (1, 3):
    # (a) / (c): forward, bias + ReLU, cin 40
    for _cout, _n, _form in ((64, 1, (1, 4)), (64, 4, (2, 2)), (64, 8, (4, 1)), (48, 8, (4, 1)), (128, 1, (1, 4)), (128, 2, (2, 2)),
                             (128, 4, (4, 1)), (128, 8, (4, 1)), (32, 1, (1, 2)), (32, 4, (1, 2)), (32, 8, (2, 1)), (24, 8, (2, 1))):
        _case(f"fwd_k{_ks}_c{_cout}_n{_n}", "conv_f32", dict(form=(_form[0], _ks, _form[1])), cout=_cout, ks=_ks, N=_n, H=FH, W=FW)
    # (b) the input gradient = this kernel with the transposed pack: `cout` is the gradient's channel count (the forward cin)
    _case(f"dgrad_k{_ks}_64_from_40", "conv_f32", dict(form=(4, _ks, 1)), cout=64, ks=_ks, N=8, H=FH, W=FW)
    _case(f"dgrad_k{_ks}_32_from_64", "conv_f32", dict(form=(2, _ks, 1)), cout=32, ks=_ks, N=8, H=FH, W=FW)
# the two edges of the rule itself: one-tile-high strips of 129 and 257 tiles
_case("edge_g129", "conv_f32", dict(form=(2, 3, 2), g=129), cout=64, ks=3, N=1, H=5, W=32 * 128 + 1)
_case("edge_g257", "conv_f32", dict(form=(4, 3, 1), g=257), cout=64, ks=3, N=1, H=5, W=32 * 256 + 1)
# (b) epilogues on <4,KS,1>
_case("epi_lff", "conv_f32", dict(form=(4, 1, 1)), cout=64, ks=1, N=8, H=FH, W=FW)
_case("epi_out2", "conv_f32", dict(form=(4, 3, 1)), cout=64, ks=3, N=8, H=FH, W=FW)
# (h) the dense 64 -> 64 3x3 layers of SuperResolutionNet(3, 2, 64, 1, 1) on 64x64 clips: B * T images per launch
_case("net_sr_b1", "conv_f32", dict(form=(1, 3, 4), g=48), cout=64, ks=3, N=1 * 3, H=64, W=64)
_case("net_sr_b8", "conv_f32", dict(form=(4, 3, 1), g=384), cout=64, ks=3, N=8 * 3, H=64, W=64)
# (d) weight gradient, N = 8: 288 tiles
_case("wgrad_32_32_k3", "wgrad_f32", dict(nsplit=288, tiles=(1, 1), chains=True, bias_trips=5), cin_w=32, cin_store=32, cout=32,
      ks=3, N=8, H=FH, W=FW)
_case("wgrad_64_64_k3", "wgrad_f32", dict(nsplit=128, tiles=(2, 3), chains=True, bias_trips=2), cin_w=64, cin_store=64, cout=64,
      ks=3, N=8, H=FH, W=FW)
_case("wgrad_81_128_k1", "wgrad_f32", dict(nsplit=40, tiles=(7, 8), chains=True, bias_trips=1), cin_w=81, cin_store=96, cout=128,
      ks=1, N=8, H=FH, W=FW)
# (e) stem: 75x75 outputs, 10 x 10 x 3 = 300 tiles on 256 workgroups
_case("stem_co64", "stem", dict(tiles=300, wg=256, two_tiles=44, per_wg=2, reduce_trips=4, passes=1, live_last=64), Co=64, N=3,
      H=149, W=149)
_case("stem_co72", "stem", dict(tiles=300, wg=256, two_tiles=44, per_wg=2, reduce_trips=4, passes=2, live_last=8), Co=72, N=3,
      H=149, W=149)
# (f) depthwise weight gradient: 17 x 16 x 2 = 544 tiles on 512 workgroups
_case("dw_f32_c32", "dw", dict(tiles=544, wg=512, per_wg=2, form="tiled", reduce_trips=8), C=32, N=2, H=129, W=481, bf16=False)
_case("dw_bf16_c64", "dw", dict(tiles=544, wg=512, per_wg=2, form="bf16_full_line", reduce_trips=8), C=64, N=2, H=129, W=481,
      bf16=True)
# (g) bf16 automatic choice
_case("auto_64_32_128x128", "bf16_auto", dict(tiles16=32, underfilled=False, same_as=162), cin=64, cout=32, H=128, W=128)
_case("auto_64_32_112x128", "bf16_auto", dict(tiles16=28, underfilled=True, same_as=8), cin=64, cout=32, H=112, W=128)
_case("auto_160_32_128x128", "bf16_auto", dict(tiles16=32, underfilled=False, same_as=16), cin=160, cout=32, H=128, W=128)

BY_NAME = {r["name"]: r for r in CASES}
assert len(BY_NAME) == len(CASES)

RULES = {
    "conv_f32": lambda c, r: conv_f32_rule(c, r["cout"], r["ks"], r["N"], r["H"], r["W"]),
    "wgrad_f32": lambda c, r: wgrad_f32_rule(c, r["cin_w"], r["cout"], r["N"], r["H"], r["W"]),
    "stem": lambda c, r: stem_rule(c, r["Co"], r["N"], r["H"], r["W"]),
    "dw": lambda c, r: dw_rule(c, r["C"], r["N"], r["H"], r["W"], r["bf16"]),
    "bf16_auto": lambda c, r: bf16_auto_rule(c, r["cin"], r["cout"], r["H"], r["W"]),
}


@pytest.fixture(scope="module")
def consts():
    return host_constants()


def test_constants_are_the_ones_the_table_was_laid_out_for(consts):
    """the frame arithmetic of the table (36 ragged tiles of 8x32, a ragged third K chunk) holds for the constants in csrc/"""
    assert (consts["TH"], consts["TW"]) == (8, 32)
    assert (cdiv(FH, consts["TH"]), FH % consts["TH"], cdiv(FW, consts["TW"]), FW % consts["TW"]) == (9, 3, 4, 1)
    assert cdiv(CIN, consts["KC"]) == 3 and CIN % consts["KC"] == 8


@pytest.mark.parametrize("row", CASES, ids=[r["name"] for r in CASES])
def test_case_reaches_its_intended_form(consts, row):
    got = RULES[row["kind"]](consts, row)
    for key, want in row["want"].items():
        assert got[key] == want, f"{row['name']}: {key} is {got[key]} for this shape, the case is meant to run {want} ({got})"


def test_every_size_selected_fp32_conv_form_is_in_the_table(consts):
    """all ten conv_f32_kernel instantiations with NT >= 32 appear, for both kernel sizes"""
    seen = {RULES["conv_f32"](consts, r)["form"] for r in CASES if r["kind"] == "conv_f32"}
    for ks in (1, 3):
        for nb, gs in ((1, 4), (2, 2), (4, 1), (1, 2), (2, 1)):
            assert (nb, ks, gs) in seen
