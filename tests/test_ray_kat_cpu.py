"""The oracle's ray routines (oracle/rt.c: Möller-Trumbore, the slab test, the
BVH walks over arbitrary rays, the PCG stream and the bounce sampler) held to
the exact model of tests/ray_reference.py and the hand-worked table of
tests/ray_known_answers.py; tests/test_gpu_ray_kat.py holds the rt_kat image
to the oracle over the same tables.  check_sensitivity shows on the model
alone that the tables tell each wrong variant of a routine from the right one.
"""
from fractions import Fraction

import numpy as np
import pytest

import ray_known_answers as ka
import ray_reference as rr
from skybox_rt_amd import rt

# bounce_dir against the float64 model: the oracle's worst |dir - dir_model|
# over the table measured 1.10e-7 (about two float32 roundings of a component
# near 1); only fp32 rounding separates the two, so the bound is 4 x that.
BOUNCE_MEASURED = 1.10e-7
BOUNCE_BOUND = 4 * BOUNCE_MEASURED


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- known answers ------------------------------------------------------------
def test_known_answers_pcg(oracle_lib):
    po = oracle_lib
    for v, want in ka.PCG_KAT:
        assert rr.pcg_hash(v) == want and int(po.pcg_hash([v])[0]) == want
    for (s, p, v), want in ka.PT_KEY_KAT:
        assert rr.pt_key(s, p, v) == want and int(po.pt_key([s], [p], [v])[0]) == want
    for h, want in ka.PT_U11_KAT:
        assert rr.pt_u11(h) == want and float(po.pt_u11([h])[0]) == want
        assert np.float32(want) == want       # the answers are float32 values


def test_known_answers_triangle(oracle_lib):
    po = oracle_lib
    o, d, v0, e1, e2, tmin = ka.mt_kat_arrays()
    hit, t = po.mt(o, d, v0, e1, e2, tmin)
    for i, row in enumerate(ka.MT_KAT):
        ok, tm, _ = rr.mt_exact(o[i], d[i], v0[i], e1[i], e2[i], tmin[i])
        assert ok == row[4] and bool(hit[i]) == row[4], i
        if row[4]:
            assert float(tm) == row[5] and float(t[i]) == row[5], i


def _slab_rows(rows, planes_of):
    o = np.array([r[0] for r in rows], np.float32)
    d = np.array([r[1] for r in rows], np.float32)
    pl = np.array([planes_of(r[2]) for r in rows], np.float32)
    tmin = np.array([r[3] for r in rows], np.float32)
    tmax = np.array([r[4] for r in rows], np.float32)
    return o, d, pl, tmin, tmax


def model_slab(o, d, pl, tmin, tmax):
    """(verdict, tnear, tfar) of the exact interval clipped to [tmin, tmax];
    tnear / tfar None where the ray misses an axis' slab altogether"""
    iv = rr.box_interval(o, d, pl[0::2], pl[1::2])
    if iv is None:
        return False, None, None
    t0, t1 = iv
    a = rr.frac(tmin) if t0 is None else max(t0, rr.frac(tmin))
    b = (None if np.isinf(tmax) else rr.frac(tmax)) if t1 is None else (t1 if np.isinf(tmax) else min(t1, rr.frac(tmax)))
    return (b is None or a <= b), a, b


def test_known_answers_box(oracle_lib):
    po = oracle_lib
    for rows, planes_of in ((ka.SLAB_KAT, lambda p: p), (ka.SLAB_HALF_KAT, ka.half_to_f32)):
        o, d, pl, tmin, tmax = _slab_rows(rows, planes_of)
        hit, tn, tf = po.slab(o, d, pl, tmin, tmax)
        for i, row in enumerate(rows):
            assert bool(hit[i]) == row[5] and float(tn[i]) == row[6] and float(tf[i]) == row[7], (i, hit[i], tn[i], tf[i])
            ok, a, b = model_slab(o[i], d[i], pl[i], tmin[i], tmax[i])
            assert ok == row[5] and a == Fraction(row[6]) and b == Fraction(row[7]), i


def _closer_scene():
    tri = np.array([ka._T, ka._T], np.float32)
    return ka.tri9_of(tri)


def test_known_answers_closer(oracle_lib):
    po = oracle_lib
    tri9 = _closer_scene()
    for tmax, tie, pid, t in ka.CLOSER_KAT:
        rays = ka.pack_rays([[1, 1, -2]], [[0, 0, 4]], [0.0], [tmax])
        p, tt, _ = po.trace_rays(tri9, rays, [-1], [tie])
        assert (int(p[0]), float(tt[0])) == (pid, t)
        inside, tl, _ = rr.lattice_hits([[1, 1, -2]], [[0, 0, 4]], tri9[:, 0:3], tri9[:, 3:6], tri9[:, 6:9])
        mp, mt, _ = rr.closest_hits(inside, tl, [0.0], [tmax], [-1], [tie])
        assert (int(mp[0]), float(mt[0])) == (pid, t)
    assert rr.closer(1.0, 3, 1.0, 5, False) and not rr.closer(1.0, 3, 1.0, 5, True)


# ---- Möller-Trumbore ------------------------------------------------------------
@pytest.fixture(scope="module")
def mt_lattice():
    o, d, v0, e1, e2, tmin = ka.mt_lattice_table()
    model = [rr.mt_exact(o[i], d[i], v0[i], e1[i], e2[i], tmin[i]) for i in range(len(o))]
    return (o, d, v0, e1, e2, tmin), model


def test_mt_lattice_exact(oracle_lib, mt_lattice):
    """verdict and t bits against the rationals: no mismatch, nothing left out"""
    (o, d, v0, e1, e2, tmin), model = mt_lattice
    hit, t = oracle_lib.mt(o, d, v0, e1, e2, tmin)
    want = np.array([m[0] for m in model])
    want_t = np.array([m[1] if m[0] else 0.0 for m in model], np.float32)
    assert int((hit.astype(bool) != want).sum()) == 0
    assert int((bits(t) != bits(want_t)).sum()) == 0
    on_edge = sum(1 for m in model if m[0] and rr.on_boundary(m[2]))
    at_tmin = sum(1 for m, tm in zip(model, tmin) if m[2] is not None and m[2][2] == rr.frac(tm)
                  and m[2][0] >= 0 and m[2][1] >= 0 and m[2][0] + m[2][1] <= 1)
    assert on_edge >= 1000 and at_tmin >= 1000, (on_edge, at_tmin)
    # the int64 form of the model (the walks' tables use it) is the same model
    n = 2000
    inside, tl, bd = rr.lattice_hits(o[:n], d[:n], v0[:n], e1[:n], e2[:n])
    for i in range(n):
        ok = bool(inside[i, i]) and tl[i, i] > tmin[i]
        assert ok == model[i][0] and (not ok or bits(tl[i, i]) == bits(model[i][1]))


# ---- slab ---------------------------------------------------------------------
def test_slab_exact_and_conservative(oracle_lib):
    o, d, pl, tmin, tmax, exact = ka.slab_table()
    hit, tn, tf = oracle_lib.slab(o, d, pl, tmin, tmax)
    hbits, hpl = ka.half_planes_outward(pl)
    hit_h, _, _ = oracle_lib.slab(o, d, hpl, tmin, tmax)
    claims = 0
    for i in range(len(o)):
        if exact[i]:
            ok, a, b = model_slab(o[i], d[i], pl[i], tmin[i], tmax[i])
            assert bool(hit[i]) == ok, i
            if a is not None and b is not None:
                assert Fraction(float(tn[i])) == a and Fraction(float(tf[i])) == b, i
        # conservative: a ray that meets the box shrunk by 2^-20 of its coordinates' size
        # within [tmin, tmax] is accepted -- over the fp32 planes and over the wider binary16 ones
        if rr.box_meets(o[i], d[i], pl[i, 0::2], pl[i, 1::2], tmin[i], tmax[i], Fraction(1, 1 << 20)):
            claims += 1
            assert hit[i] and hit_h[i], i
    assert claims >= 500 and int(exact.sum()) >= 1000 and 0 < int(hit[exact].sum()) < int(exact.sum())
    assert np.isinf(hpl).any()


# ---- walks ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("ray_kat")


def model_walk(case):
    lat = case["lat"]
    r = case["rays"]
    return rr.closest_hits(lat["inside"], lat["t"], r[:, 6], r[:, 7], case["skip"], case["tie"])


@pytest.mark.parametrize("name", ka.WALK_SCENES)
def test_walks_equal_brute_force_and_model(oracle_lib, scene_dir, name):
    po = oracle_lib
    case = ka.walk_case(name, scene_dir, po, rt)
    r, skip, tie = case["rays"], case["skip"], case["tie"]
    bp, bt, bo = po.trace_rays(case["tri9"], r, skip, tie)
    assert (bp >= 0).sum() > 500 and (bp < 0).sum() > 200 and bo.sum() > 500
    for tname, (nodes, tris, n4, _, _) in case["trees"].items():
        for mode in (1, 2):
            p, t, occ = po.trace_rays(case["tri9"], r, skip, tie, bvh=(nodes, tris, n4), mode=mode)
            assert np.array_equal(p, bp) and np.array_equal(bits(t), bits(bt)), (tname, mode)
            assert np.array_equal(occ, bo), (tname, mode)
    if name == "chain":
        assert 24 < case["trees"]["sah"][4] <= 32
    if name == "soup_big":
        assert case["geom_inf"]          # planes past binary16's range
    if name == "soup_small":
        assert case["half_denormal"]     # planes among binary16's denormals
    if case["lat"] is not None:
        mp, mt, mo = model_walk(case)
        assert np.array_equal(mp, bp) and np.array_equal(bits(mt), bits(bt)) and np.array_equal(mo, bo.astype(bool))
        lat = case["lat"]
        won = lat["boundary"][np.arange(len(bp)), np.maximum(bp, 0)] & (bp >= 0)
        ties = (r[:, 7] == bt) & (bp >= 0)
        assert won.sum() >= 300 and ties.sum() >= 20, (won.sum(), ties.sum())
        zero = (r[:, 3:6] == 0).sum(1)
        assert (zero == 1).sum() >= 256 and (zero == 2).sum() >= 256


# ---- PCG and the sampler --------------------------------------------------------
def test_pcg_stream_bit_for_bit(oracle_lib):
    po = oracle_lib
    v = ka.pcg_inputs()
    assert np.array_equal(po.pcg_hash(v), np.array([rr.pcg_hash(int(x)) for x in v], np.uint32))
    want = np.array([rr.pt_u11(int(x)) for x in v])
    assert np.array_equal(po.pt_u11(v).astype(np.float64), want)     # every value is a float32
    k = ka.pt_key_inputs()
    assert np.array_equal(po.pt_key(k[:, 0], k[:, 1], k[:, 2]),
                          np.array([rr.pt_key(int(a), int(b), int(c)) for a, b, c in k], np.uint32))


def bounce_errors(dirs, normals, keys, cls):
    """per accepted record: |dir - dir_model|, ||dir| - 1|, |dir . n - z|, and the
    tangential part against x t1 + y t2 in the routine's own basis"""
    out = []
    for i in np.flatnonzero(cls > 0):
        n = normals[i].astype(np.float64)
        dm, x, y, z = rr.bounce_model(normals[i], int(keys[i]))
        dv = dirs[i].astype(np.float64)
        t1, t2 = rr.duff_basis(normals[i])
        tang = dv - z * n
        # (|dir| = 1 and dir . n = z are claims about unit normals: the table's (0, 0, -0.0),
        # there for the sign test's branch, is held to the model's direction only)
        unit = abs(np.linalg.norm(n) - 1.0) < 1e-6
        out.append((np.abs(dv - dm).max(), abs(np.linalg.norm(dv) - 1.0) if unit else 0.0,
                    abs(dv @ n - z) if unit else 0.0, np.abs(tang - (x * t1 + y * t2)).max()))
    return np.array(out)


def test_bounce_dir_fallback_and_accepted(oracle_lib):
    normals, keys, cls = ka.bounce_table()
    fb, acc = ka.bounce_keys()
    assert len(fb) >= 32 and all(len(acc[k]) >= 8 for k in range(1, 9))
    assert set(fb.tolist()) <= set(keys[cls == 0].tolist())
    dirs = oracle_lib.pt_bounce_dir(normals, keys)
    # a fall-back key returns n itself
    f = cls == 0
    assert np.array_equal(dirs[f], normals[f])
    err = bounce_errors(dirs, normals, keys, cls)
    print("bounce_dir worst |dir - model| %.3e, ||dir| - 1| %.3e, |dir.n - z| %.3e, tangential %.3e; bound %.3e"
          % (*err.max(0), BOUNCE_BOUND))
    assert err.max() <= BOUNCE_BOUND
    # the routine's basis is orthonormal about n (an independent Gram-Schmidt pair spans the
    # same plane: the tangential part has length sqrt(x^2 + y^2) in it)
    for i in np.flatnonzero(cls > 0)[::37]:
        n = normals[i].astype(np.float64)
        if abs(np.linalg.norm(n) - 1.0) > 1e-6:
            continue
        n /= np.linalg.norm(n)
        _, x, y, z = rr.bounce_model(normals[i], int(keys[i]))
        g1, g2 = rr.gram_schmidt_basis(n)
        tang = dirs[i].astype(np.float64) - z * normals[i].astype(np.float64)
        assert abs(np.hypot(tang @ g1, tang @ g2) - np.hypot(x, y)) <= BOUNCE_BOUND
        assert abs(tang @ n) <= BOUNCE_BOUND


# ---- sensitivity: the tables tell each wrong routine from the right one ----------
def check_sensitivity(mt_table, mt_model, soup, quads):
    """-> {mutant: records of the tables on which it differs from the model}"""
    o, d, v0, e1, e2, tmin = mt_table
    out = {}
    some = range(0, len(o), 7)     # every class of the table
    out["exclusive edges"] = sum(rr.mt_exact(o[i], d[i], v0[i], e1[i], e2[i], tmin[i], inclusive=False)[0]
                                 != mt_model[i][0] for i in some)
    out["t >= tmin"] = sum(rr.mt_exact(o[i], d[i], v0[i], e1[i], e2[i], tmin[i], strict_tmin=False)[0]
                           != mt_model[i][0] for i in some)
    lat, r = soup["lat"], soup["rays"]
    base = rr.closest_hits(lat["inside"], lat["t"], r[:, 6], r[:, 7], soup["skip"], soup["tie"])
    for key, kw in (("dropped skip", dict(use_skip=False)), ("opposite tie_high", dict(flip_tie=True))):
        m = rr.closest_hits(lat["inside"], lat["t"], r[:, 6], r[:, 7], soup["skip"], soup["tie"], **kw)
        out[key] = int(((m[0] != base[0]) | (bits(m[1]) != bits(base[1]))).sum())
    # a triangle's box (its corners' extremes: integers, binary16 values) shrunk by one
    # binary16 quantum a side: some ray that hits the triangle then misses its box
    missed = 0
    for case in (soup, quads):
        lat, r = case["lat"], case["rays"]
        bp = rr.closest_hits(lat["inside"], lat["t"], r[:, 6], r[:, 7], case["skip"], case["tie"])[0]
        for i in np.flatnonzero(bp >= 0)[:400]:
            c = lat["tri"][bp[i]].astype(np.float32)
            lo, hi = c.min(0), c.max(0)
            q = np.maximum(np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(np.float16)).astype(np.float32),
                           np.float32(2.0 ** -24))
            assert rr.box_meets(lat["o"][i], lat["d"][i], lo, hi, 0.0, np.inf)
            lo2, hi2 = lo + q, hi - q
            if np.any(lo2 > hi2) or not rr.box_meets(lat["o"][i], lat["d"][i], lo2, hi2, 0.0, np.inf):
                missed += 1
    out["box shrunk by a binary16 quantum"] = missed
    normals, keys, cls = ka.bounce_table()
    stream = last = 0
    for i in range(0, len(keys), 3):
        dm = rr.bounce_model(normals[i], int(keys[i]))[0]
        if cls[i] > 1 and np.abs(rr.bounce_model(normals[i], int(keys[i]), pair_stride=1)[0] - dm).max() > BOUNCE_BOUND:
            stream += 1
        if cls[i] == 0 and np.abs(rr.bounce_model(normals[i], int(keys[i]), fallback="last")[0] - dm).max() > BOUNCE_BOUND:
            last += 1
    out["stream read as key + i"] = stream
    out["fall-back to the last rejected pair"] = last
    return out


def test_check_sensitivity(oracle_lib, scene_dir, mt_lattice):
    soup = ka.walk_case("soup", scene_dir, oracle_lib, rt)
    quads = ka.walk_case("quads", scene_dir, oracle_lib, rt)
    res = check_sensitivity(mt_lattice[0], mt_lattice[1], soup, quads)
    print(sorted(res.items()))
    assert len(res) == 7 and all(v > 0 for v in res.values()), res
