"""The device's two restatements of the texture sampler held to the
independent model (tests/tex_reference.py) over the sweeps of
tests/tex_sweep.py and the hand-worked table (tests/tex_known_answers.py),
bit for bit:

* the RT path's gfx::tex_read (-> tex_read_fmt<FMT>) and gfx::tex_read_any
  (gfx_device.h), run by the tex_kat image over the whole unit sweep in one
  launch -- every format x filter x (wrapu, wrapv) pair, coordinates far
  outside [0, 1): states no scene can express;
* the texture kernel (tex_kernel.hip, one image per filter), driven through
  the Vortex C ABI with its argument block packed here as rt_tex_configure
  packs it, but with explicit coordinate tables, lod and frac.

tests/test_tex_unit_cpu.py holds the oracle to the same model."""
import os
import struct

import numpy as np
import pytest

import tex_known_answers as ka
import tex_reference as tr
import tex_sweep as ts

pytestmark = pytest.mark.gpu

from skybox_rt_amd import _lib, vortex  # noqa: E402

SENTINEL = 0xDEADBEEF


def _align(n, a=64):
    return (n + a - 1) // a * a


class Blob:
    """byte strings laid out in one device buffer, each at a 64-byte boundary"""

    def __init__(self):
        self.parts, self.offs, self.size = [], {}, 0

    def add(self, key, data):
        if key not in self.offs:
            data = bytes(data)
            self.offs[key] = self.size
            self.parts.append(data + bytes(_align(len(data)) - len(data)))
            self.size += len(self.parts[-1])
        return self.offs[key]

    def upload(self, dev):
        return dev.upload_bytes(b"".join(self.parts) or bytes(64))


# ---- gfx::tex_read / tex_read_any through the tex_kat image ---------------------
def run_tex_kat(recs):
    """recs: (texture key, bytes, logw, logh, fmt, filt, wrapu, wrapv, u[], v[]) per
    sampler state -> list of uint32 [n, 2] (tex_read, tex_read_any), one launch"""
    blob = Blob()
    for r in recs:
        blob.add(r[0], np.asarray(r[1], np.uint8).tobytes())
    d = vortex.Device()
    try:
        k = d.upload_kernel_file(os.path.join(_lib.LIB_DIR, "tex_kat.vxbin"))
        texbuf = blob.upload(d)
        base = texbuf.address
        assert base + blob.size < 1 << 32
        rows = []
        for key, _, logw, logh, fmt, filt, wu, wv, u, v in recs:
            u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
            t = np.zeros((u.size, 10), np.int64)
            t[:, :8] = (base + blob.offs[key], logw, logh, fmt, filt, wu, wv, tr.STRIDE[fmt])
            t[:, 8], t[:, 9] = u, v
            rows.append(t)
        table = np.concatenate(rows)
        n = table.shape[0]
        words = (table & 0xFFFFFFFF).astype(np.uint32)
        recbuf = d.upload_bytes(words.tobytes())
        out = d.upload_bytes(np.full(2 * n, SENTINEL, np.uint32).tobytes())
        args = d.upload_bytes(struct.pack("<QQII", recbuf.address, out.address, n, 0))
        d.start(k, args)
        d.ready_wait()
        o = np.frombuffer(out.read(), np.uint32).reshape(n, 2)
    finally:
        d.close()
    res, at = [], 0
    for t in rows:
        res.append(o[at:at + t.shape[0]])
        at += t.shape[0]
    return res


def test_rt_sampler_equals_model_unit_sweep():
    states = ts.unit_states()
    got = run_tex_kat([((s.shape, s.fmt), s.tex, s.logw, s.logh, s.fmt, s.filt, s.wrapu, s.wrapv,
                        s.u, s.v) for s in states])
    n = 0
    for s, g, exp in zip(states, got, ts.unit_expected()):
        for col, name in enumerate(("tex_read", "tex_read_any")):
            bad = np.flatnonzero(g[:, col] != exp)
            assert bad.size == 0, (
                f"gfx::{name} state {s.key()}: {bad.size} samples differ, first u={s.u[bad[0]]} "
                f"v={s.v[bad[0]]} device {g[bad[0], col]:#010x} model {exp[bad[0]]:#010x}")
        n += exp.size
    assert n == ts.UNIT_SAMPLES


def test_rt_sampler_reproduces_known_answers():
    rows = [r for r in ka.SAMPLES if r[6] != tr.TRILINEAR and r[11] == 0]
    assert len(rows) >= 24
    got = run_tex_kat([(r[0], r[1], r[3], r[4], r[5], r[6], r[7], r[8], [r[9]], [r[10]]) for r in rows])
    for r, g in zip(rows, got):
        assert int(g[0, 0]) == r[-1], f"{r[0]}: tex_read {int(g[0, 0]):#010x}"
        assert int(g[0, 1]) == r[-1], f"{r[0]}: tex_read_any {int(g[0, 1]):#010x}"


# ---- the texture kernel, one image per filter -------------------------------------
def tex_group(filt):
    """tex_common.h TEX_GROUP: pixels of a row one wave owns"""
    return 64 * (8 if filt == 0 else 4)


def run_tex_kernel(filt, jobs):
    """jobs: (texture key, bytes, mipoff, logw, logh, fmt, wrap, lod, frac, table key,
    utab, vtab) per destination image, all for filter image `filt` -> list of
    (image uint32 [dh, dw], guard uint32[]: the padded row after the image, which
    must still hold SENTINEL).  One device, one launch per job."""
    grp = tex_group(filt)
    texs, tabs = Blob(), Blob()
    layout, dst_words = [], 0
    for key, tex, _, _, _, _, _, _, _, tkey, utab, vtab in jobs:
        texs.add(key, np.asarray(tex, np.uint8).tobytes())
        dw, dh = len(utab), len(vtab)
        gpr = (dw + grp - 1) // grp
        padded = np.zeros(gpr * grp, np.int64)        # rt_tex_configure: whole groups, zeros past dw
        padded[:dw] = utab
        uo = tabs.add(("u", tkey, dw), (padded & 0xFFFFFFFF).astype(np.uint32).tobytes())
        vo = tabs.add(("v", tkey), (np.asarray(vtab, np.int64) & 0xFFFFFFFF).astype(np.uint32).tobytes())
        layout.append((dst_words, dw, dh, gpr, uo, vo))
        dst_words += dw * dh + gpr * grp              # the image, then a guard row of a padded row
    d = vortex.Device()
    try:
        k = d.upload_kernel_file(os.path.join(_lib.LIB_DIR, f"tex_kernel_f{filt}.vxbin"))
        texbuf, tabbuf = texs.upload(d), tabs.upload(d)
        dst = d.upload_bytes(np.full(dst_words, SENTINEL, np.uint32).tobytes())
        assert dst.address + 4 * dst_words < 1 << 32
        args = d.mem_alloc(256)
        for job, (off, dw, dh, gpr, uo, vo) in zip(jobs, layout):
            key, _, mipoff, logw, logh, fmt, wrapm, lod, frac = job[:9]
            mip = [int(x) for x in mipoff] + [0] * (16 - len(mipoff))
            args.write(struct.pack("<4Q10I16I", dst.address + 4 * off, tabbuf.address + uo,
                                   tabbuf.address + vo, texbuf.address + texs.offs[key], dw, dh, filt,
                                   lod, frac, logw, logh, fmt, wrapm, dh * gpr * 64, *mip))
            d.start(k, args)
            d.ready_wait()
        o = np.frombuffer(dst.read(), np.uint32)
    finally:
        d.close()
    return [(o[off:off + dw * dh].reshape(dh, dw), o[off + dw * dh:off + dw * dh + gpr * grp])
            for off, dw, dh, gpr, _, _ in layout]


@pytest.mark.parametrize("filt", [0, 1, 2])
def test_tex_kernel_equals_model_image_sweep(filt):
    cases = list(ts.image_cases(filt))
    assert len(cases) == ts.IMAGE_CASES // 6 * (4 if filt == 2 else 1)
    got = run_tex_kernel(filt, [((t.index, t.fmt), t.tex, t.mipoff, t.logw, t.logh, t.fmt, wrapm, lod,
                                 frac, t.index, t.utab[:dw], t.vtab)
                                for t, wrapm, _, frac, lod, dw in cases])
    for (t, wrapm, _, frac, lod, dw), (img, guard) in zip(cases, got):
        what = f"texture {t.w}x{t.h} fmt {t.fmt} wrap {wrapm} lod {lod} frac {frac} width {dw}"
        exp = ts.image_expected(t, wrapm, filt, frac, lod, dw)
        assert np.array_equal(img, exp), f"{what}: {int((img != exp).sum())} pixels differ"
        assert np.all(guard == SENTINEL), f"{what}: written past the image"


def test_tex_kernel_reproduces_known_answers():
    """the rows a single wrap mode can express, each as a 1x1 destination"""
    for filt in (0, 1, 2):
        rows = [r for r in ka.SAMPLES if r[6] == filt and r[7] == r[8]]
        assert rows
        got = run_tex_kernel(filt, [(r[0], r[1], r[2], r[3], r[4], r[5], r[7], r[11], r[12], r[0],
                                     [r[9]], [r[10]]) for r in rows])
        for r, (img, guard) in zip(rows, got):
            assert int(img[0, 0]) == r[-1], f"{r[0]}: {int(img[0, 0]):#010x}"
            assert np.all(guard == SENTINEL), r[0]
