"""The texture sampler held to an independent model on the CPU: the model
(tests/tex_reference.py) reproduces the hand-worked table
(tests/tex_known_answers.py); the oracle's sampler (orc_tex_read), its
renders (orc_tex_render, orc_tex_render_tab), its lod and both mip-chain
builders (the oracle's and the product host's) equal the model over the full
sweeps (tests/tex_sweep.py).  Everything is integer arithmetic: the tolerance
is 0.  tests/test_gpu_tex_unit.py holds the device to the same model."""
import itertools

import numpy as np
import pytest

import tex_known_answers as ka
import tex_reference as tr
import tex_sweep as ts


def model_sample(row):
    _, tex, mip, logw, logh, fmt, filt, wu, wv, u, v, lod, frac, _ = row
    tex = np.array(tex, np.uint8)
    mipoff = np.zeros(16, np.int64)
    mipoff[:len(mip)] = mip
    if filt == tr.TRILINEAR:
        return int(tr.read_trilinear(tex, mipoff, logw, logh, fmt, wu, wv, [u], [v], lod, frac)[0])
    return int(tr.read(tex, mipoff, logw, logh, fmt, filt, wu, wv, [u], [v], lod)[0])


def test_model_reproduces_known_answers():
    assert len(ka.WRAPS) + len(ka.SAMPLES) + len(ka.LODS) >= 24
    for name, mode, d, exp in ka.WRAPS:
        assert int(tr.wrap(d, mode)) == exp, name
    for row in ka.SAMPLES:
        assert model_sample(row) == row[-1], f"{row[0]}: {model_sample(row):#010x}"
    for name, logw, logh, dw, dh, lod, frac in ka.LODS:
        assert tr.lod_frac(logw, logh, dw, dh) == (lod, frac), name


def test_oracle_reproduces_known_answers(oracle_lib):
    po = oracle_lib
    for row in ka.SAMPLES:
        name, tex, mip, logw, logh, fmt, filt, wu, wv, u, v, lod, frac, exp = row
        mipoff = np.zeros(16, np.uint32)
        mipoff[:len(mip)] = mip
        if filt != tr.TRILINEAR and lod == 0:
            got = int(po.tex_read(tex, logw, logh, fmt, filt, wu, wv, [u], [v])[0])
            assert got == exp, f"{name}: orc_tex_read {got:#010x}"
        if wu == wv:
            got = int(po.tex_render_tab(tex, mipoff, logw, logh, fmt, wu, filt, lod, frac, [u], [v])[0, 0])
            assert got == exp, f"{name}: orc_tex_render_tab {got:#010x}"
        else:
            assert filt != tr.TRILINEAR
    for name, logw, logh, dw, dh, lod, frac in ka.LODS:
        assert po.tex_lod(logw, logh, dw, dh) == (lod, frac), name


def test_oracle_equals_model_unit_sweep(oracle_lib):
    po = oracle_lib
    n = 0
    for s, exp in zip(ts.unit_states(), ts.unit_expected()):
        got = po.tex_read(s.tex, s.logw, s.logh, s.fmt, s.filt, s.wrapu, s.wrapv, s.u, s.v)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (f"state {s.key()}: {bad.size} samples differ, first u={s.u[bad[0]]} "
                               f"v={s.v[bad[0]]} oracle {got[bad[0]]:#010x} model {exp[bad[0]]:#010x}")
        n += exp.size
    assert n == ts.UNIT_SAMPLES and 50_000 <= n <= 100_000


def test_oracle_equals_model_image_sweep(oracle_lib):
    po = oracle_lib
    n = 0
    for t, wrapm, filt, frac, lod, dw in ts.image_cases():
        got = po.tex_render_tab(t.tex, t.mipoff, t.logw, t.logh, t.fmt, wrapm, filt, lod, frac,
                                t.utab[:dw], t.vtab)
        exp = ts.image_expected(t, wrapm, filt, frac, lod, dw)
        assert np.array_equal(got, exp), (t.index, t.fmt, wrapm, filt, frac, lod, dw)
        n += 1
    assert n == ts.IMAGE_CASES


def _images():
    rng = np.random.default_rng(ts.SEED + 3)
    return {wh: rng.integers(0, 1 << 32, wh[::-1], dtype=np.uint64).astype(np.uint32)
            for wh in ((16, 16), (32, 8), (8, 32), (1, 8), (1, 1))}


SCALES = (0.3, 0.77, 1.0, 1.37, 2.0)


@pytest.mark.parametrize("wh", [(16, 16), (32, 8), (8, 32)])
def test_oracle_app_render_equals_model(oracle_lib, wh):
    """orc_tex_render (float coordinates accumulated per column and per task
    tile, lod / frac from the minification, the oracle's own chain) against
    the model's replay, every format x wrap x filter x scale"""
    po = oracle_lib
    src = _images()[wh]
    for fmt in range(7):
        chain = tr.build_chain(src, fmt)
        for wrapm, filt, scale in itertools.product(range(3), range(3), SCALES):
            got = po.tex_render(src, fmt=fmt, wrap=wrapm, filt=filt, scale=scale)
            exp = tr.render_app(src, fmt, wrapm, filt, scale, chain=chain)
            assert np.array_equal(got, exp), (fmt, wrapm, filt, scale)


@pytest.mark.parametrize("num_tasks", [1, 7])
def test_oracle_app_render_task_tiles(oracle_lib, num_tasks):
    """v restarts at every task's first row: 21 rows in tiles of 21 / 3"""
    po = oracle_lib
    src = _images()[16, 16]
    for fmt, filt in itertools.product((0, 1, 6), range(3)):
        got = po.tex_render(src, fmt=fmt, wrap=1, filt=filt, scale=1.37, num_tasks=num_tasks)
        assert got.shape == (21, 21)
        assert np.array_equal(got, tr.render_app(src, fmt, 1, filt, 1.37, num_tasks=num_tasks)), (fmt, filt)


def test_oracle_lod_equals_model(oracle_lib):
    """over a grid that includes ratios of 2^15 and above, where the lod would
    clamp to 15 if the fixed-point word did not saturate first (row lod_sat)"""
    po = oracle_lib
    logs = (0, 1, 3, 5, 8, 12, 14, 15, 16)
    dims = (1, 2, 3, 5, 7, 12, 16, 100, 257, 1000)
    seen = set()
    for logw, logh, dw, dh in itertools.product(logs, logs, dims, dims):
        m = tr.lod_frac(logw, logh, dw, dh)
        assert po.tex_lod(logw, logh, dw, dh) == m, (logw, logh, dw, dh)
        seen.add(m[0])
    assert seen == set(range(15))     # every reachable lod; 15 is not (lod_sat)


@pytest.mark.parametrize("wh", [(16, 16), (32, 8), (1, 8), (1, 1)])
def test_mip_builders_equal_model(oracle_lib, wh):
    """the oracle's and the product host's image conversion + mip chain
    against the model's encode and 2x2 box chain, every format"""
    from skybox_rt_amd import tex
    po = oracle_lib
    src = _images()[wh]
    for fmt in range(7):
        texels, mipoff, levels = tr.build_chain(src, fmt)
        for who, (b, m, lv) in (("oracle", po.tex_build(src, fmt)), ("host", tex.build_image(src, fmt))):
            assert lv == levels, (who, fmt)
            assert np.array_equal(np.asarray(m, np.int64), mipoff), (who, fmt)
            assert np.array_equal(b, texels), (who, fmt)


def test_sweeps_tell_the_states_apart():
    ts.check_sensitivity()
