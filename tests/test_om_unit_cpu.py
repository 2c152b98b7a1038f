"""The oracle's output merger (oracle/gfx.c orc_om_write, through orc_om_app)
against the independent numpy model of the unit (tests/om_reference.py), bit
for bit on both planes, over the state sweep of tests/om_sweep.py; the model
against the hand-worked known answers (tests/om_known_answers.py); and proof,
on the model alone, that the sweep's inputs tell a subtly wrong unit from a
right one.

States x pixels compared here: blend 280 x 65 536, logic op 50 x 65 536,
depth/stencil 3 072 x 2 048 (two planes each)."""
import itertools

import numpy as np
import pytest

import om_reference as R
import om_sweep as S
from om_known_answers import KNOWN_ANSWERS


def _mismatches(case, po):
    rc, rz = S.reference(case)
    oc, oz = S.oracle(po, case)
    return int((rc != oc).sum()) + int((rz != oz).sum())


# ---- the model reproduces the hand table; so does the oracle ----
@pytest.mark.parametrize("kat", KNOWN_ANSWERS, ids=[k[0] for k in KNOWN_ANSWERS])
def test_reference_reproduces_known_answer(kat):
    _, kw, back, src, depth, c0, z0, c1, z1 = kat
    c, z = R.om_reference(R.make_dcr(**kw), back, src, depth, np.array([[c0]], np.uint32),
                          np.array([[z0]], np.uint32))
    assert (hex(int(c[0, 0])), hex(int(z[0, 0]))) == (hex(c1), hex(z1))


def test_oracle_reproduces_known_answers(oracle_lib):
    """a 1 x 256 frame with num_tasks = 256: row y has source alpha
    (y * 255) & 0xff = -y & 0xff, so row -alpha & 0xff is the entry's pixel"""
    for name, kw, back, src, depth, c0, z0, c1, z1 in KNOWN_ANSWERS:
        c, z = S.oracle_app(oracle_lib, R.make_dcr(**kw), back, True, 256, src & 0xFFFFFF, depth,
                            np.full((256, 1), c0, np.uint32), np.full((256, 1), z0, np.uint32))
        a = -(src >> 24) & 0xFF
        assert (hex(int(c[a, 0])), hex(int(z[a, 0]))) == (hex(c1), hex(z1)), name


def test_alpha_ramp():
    # every row a task: alpha = (y * 255) & 0xff = -y & 0xff, each value once in 256 rows
    y = np.arange(256, dtype=np.int64)
    assert np.array_equal(R.alpha_ramp(256, 256, 0x123456)[:, 0].astype(np.int64),
                          (((y * 255) & 0xFF) << 24) | 0x123456)
    # 3 * H tasks of one row: the same ramp; H = 37 in 7 tasks: 6 rows per task, 255 / 6 per step
    assert np.array_equal(R.alpha_ramp(37, 111, 0), R.alpha_ramp(37, 37, 0))
    assert [int(v) >> 24 for v in R.alpha_ramp(37, 7, 0)[::6, 0]] == [0, 42, 85, 127, 170, 212, 255]
    # alpha bits above 8 fall off the colour word: tile_h = 1, task 300 -> 76500 & 0xff
    assert int(R.alpha_ramp(301, 301, 0)[300, 0]) >> 24 == (300 * 255) & 0xFF


# ---- the sweep: oracle == model ----
def test_blend_arithmetic_sweep(oracle_lib):
    cases = S.blend_cases()
    assert len(cases) == 280
    bad = [c.name for c in cases if _mismatches(c, oracle_lib)]
    assert bad == []


def test_logic_op_sweep(oracle_lib):
    cases = S.logic_cases()
    assert len(cases) == 50
    bad = [c.name for c in cases if _mismatches(c, oracle_lib)]
    assert bad == []


@pytest.mark.parametrize("backface", (0, 1), ids=("front", "back"))
def test_depth_stencil_sweep(oracle_lib, backface):
    bad, n = [], 0
    for f in range(8):
        for c in S.ds_cases(backface, f):
            n += 1
            if _mismatches(c, oracle_lib):
                bad.append(c.name)
    assert n == 1536 and bad == []


def test_sweep_covers_what_it_claims():
    blend = S.blend_cases()
    for m in (R.ADD, R.SUB, R.REV_SUB):
        mine = [c for c in blend if int(c.dcr[R.BLEND_MODE]) == (m | (m << 16))]
        for pos in (0, 16):     # source rgb, destination rgb
            assert {(int(c.dcr[R.BLEND_FUNC]) >> pos) & 0xFF for c in mine} == set(range(15))
    mixed = [c for c in blend if c.name.startswith("mixed")]
    assert len(mixed) >= 6
    for c in mixed:
        f, m = int(c.dcr[R.BLEND_FUNC]), int(c.dcr[R.BLEND_MODE])
        assert len({f & 0xFF, (f >> 8) & 0xFF, (f >> 16) & 0xFF, f >> 24}) == 4
        assert (m & 0xFFFF) != (m >> 16)
    const = int(blend[0].dcr[R.BLEND_CONST])
    assert len({(const >> s) & 0xFF for s in (0, 8, 16, 24)}) == 4
    logic = S.logic_cases()
    assert {(int(c.dcr[R.LOGIC_OP]), int(c.dcr[R.CBUF_WRITEMASK])) for c in logic} >= \
        {(op, m) for op in range(16) for m in (0xF, 0x5, 0x0)}
    halves = {(int(c.dcr[R.BLEND_MODE]) & 0xFFFF == R.LOGICOP, int(c.dcr[R.BLEND_MODE]) >> 16 == R.LOGICOP)
              for c in logic}
    assert {(True, False), (False, True)} <= halves
    for slot in range(3):       # every operation in every slot
        assert {t[slot] for t in S.DS_TRIPLES} == set(range(8))
    # the two halves of every stencil word differ
    for c in S.ds_cases(0, R.LESS) + S.ds_cases(1, R.LESS):
        for w in range(R.STENCIL_FUNC, R.STENCIL_WRITEMASK + 1):
            assert int(c.dcr[w]) & 0xFFFF != int(c.dcr[w]) >> 16, (c.name, w)
    # blend frame: every (source alpha, destination byte) pair, once
    c0, _ = S.frame("blend")
    a = S.source_color(blend[0]) >> np.uint32(24)
    pairs = (a.astype(np.int64) << 8) | (c0 & 0xFF)
    assert len(np.unique(pairs)) == 65536
    assert all(np.array_equal((c0 >> np.uint32(s)) & 0xFF, c0 & 0xFF) for s in (8, 16, 24))


# ---- discrimination, on the model alone ----
def _frames_differ(a, b):
    return int((a[0] != b[0]).sum()) + int((a[1] != b[1]).sum())


def _blend(mode, func):
    return S.Case("probe", "blend", R.make_dcr(mode=mode, func=func, const=S.BLEND_CONST),
                  blend_enable=True, rgb=S.BLEND_RGB)


@pytest.mark.parametrize("variant,case", [
    ("trunc", _blend((R.ADD, R.ADD), (R.F_SRC_A, R.F_SRC_A, R.F_ONE_MINUS_SRC_A, R.F_ONE_MINUS_SRC_A))),
    ("no_round", _blend((R.ADD, R.ADD), (R.F_SRC_A, R.F_SRC_A, R.F_ONE_MINUS_SRC_A, R.F_ONE_MINUS_SRC_A))),
    ("no_round", _blend((R.SUB, R.SUB), (R.F_ONE, R.F_ONE, R.F_SRC_A, R.F_SRC_A))),
    ("no_clamp", _blend((R.ADD, R.ADD), (R.F_ONE, R.F_ONE, R.F_ONE, R.F_ONE))),
    ("face_swap", S.ds_case(0, R.LESS, R.EQUAL, S.DS_TRIPLES[2], S.DS_MASKS[0])),
    ("face_swap", S.ds_case(1, R.LESS, R.EQUAL, S.DS_TRIPLES[2], S.DS_MASKS[0])),
], ids=("trunc", "no_round_add", "no_round_sub", "no_clamp", "face_swap_front", "face_swap_back"))
def test_a_wrong_unit_changes_pixels(variant, case):
    assert _frames_differ(S.reference(case), S.reference(case, variant=variant)) > 0


def test_every_sweep_family_catches_every_wrong_unit():
    """... and not only on hand-picked states: a sample of the sweep's own
    states shows each arithmetic slip and the face swap"""
    blend = S.blend_cases()[::7]
    for variant in ("trunc", "no_round", "no_clamp"):
        hit = sum(_frames_differ(S.reference(c), S.reference(c, variant=variant)) > 0 for c in blend)
        assert hit > 0, variant
    ds = S.ds_cases(0, R.LEQUAL)[::5]
    assert sum(_frames_differ(S.reference(c), S.reference(c, variant="face_swap")) > 0 for c in ds) > 0


def _pairwise_different(results):
    for (i, a), (j, b) in itertools.combinations(enumerate(results), 2):
        assert _frames_differ(a, b) > 0, (i, j)


def test_depth_stencil_frame_separates_the_compare_functions():
    c0, z0 = S.frame("ds")
    src = S.DS_COLOR | 0xFF000000
    # as the depth function (stencil off)
    _pairwise_different([R.om_reference(R.make_dcr(cmask=0xA, depth_func=f, depth_wm=1), False, src,
                                        S.DS_DEPTH, c0, z0) for f in range(8)])
    # as the stencil function (depth off), through the colour plane alone and
    # through the stencil plane alone
    res = [R.om_reference(R.make_dcr(cmask=0xA, stencil_func=(f, 0), zpass=(R.INVERT, 0),
                                     fail=(R.ZERO, 0), ref=(0x6B, 0), mask=(0xFF, 0), swm=(0xFF, 0)),
                          False, src, S.DS_DEPTH, c0, z0) for f in range(8)]
    _pairwise_different(res)
    for plane in (0, 1):
        _pairwise_different([(r[plane], r[plane]) for r in res])


def test_depth_stencil_frame_separates_the_stencil_ops():
    c0, z0 = S.frame("ds")
    for slot in ("zpass", "zfail", "fail"):
        # zpass: everything passes; zfail: depth NEVER; fail: stencil NEVER
        kw = dict(zpass=dict(), zfail=dict(depth_func=R.NEVER), fail=dict(stencil_func=(R.NEVER, 0)))[slot]
        res = []
        for op in range(8):
            # the other two slots are never chosen; ZERO there keeps the stencil on
            ops = dict(zpass=(R.ZERO, 0), zfail=(R.ZERO, 0), fail=(R.ZERO, 0))
            ops[slot] = (op, 0)
            res.append(R.om_reference(R.make_dcr(cmask=0xA, ref=(0x6B, 0), mask=(0xFF, 0), swm=(0xFF, 0),
                                                 **kw, **ops), False, S.DS_COLOR, S.DS_DEPTH, c0, z0))
        _pairwise_different([(r[1], r[1]) for r in res])
