"""The ray routines of kernels/rt_trace.h and kernels/rt_path.h on the device
(the rt_kat image, run through the Vortex C ABI) over the tables of tests/
ray_known_answers.py: Möller-Trumbore, the slab test and the PCG sampler bit
for bit the oracle's (which tests/test_ray_kat_cpu.py holds to the exact
model), and every BVH walk -- trace closest and any over BVH2, fp32 BVH4 and
binary16 BVH4, occluded_packet, trace_coop -- equal to the device's own brute
force (trace_flat_range over every triangle) and to the oracle's, per active
lane, under four activity patterns; inactive lanes' slots and the guard words
behind every output stay as filled."""
import os
import struct

import numpy as np
import pytest

import ray_known_answers as ka

pytestmark = pytest.mark.gpu

from skybox_rt_amd import _lib, rt, vortex  # noqa: E402

MT, SLAB, WALK, PT = 0, 1, 2, 3
REC = {MT: 16, SLAB: 20, WALK: 12, PT: 20}
OUT = {MT: 4, SLAB: 8, WALK: 12, PT: 12}
FILL = 0xA5A5A5A5
GUARD = 256
RT_FLAG_BVH4, RT_FLAG_BVH4H = 0x40, 0x80


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Kat:
    """one device with the rt_kat image (every BVH layout, the 32-entry stack), or rt_kat_pt:
    the same file under the path tracer's defines -- the binary16 BVH4 only, unconditional push
    rows, the pair walk's one-exchange node step and prefetch, the 24-entry stack"""

    def __init__(self, image="rt_kat"):
        self.image = image
        self.stack = 32 if image == "rt_kat" else 24
        self.d = vortex.Device()
        self.k = self.d.upload_kernel_file(os.path.join(_lib.LIB_DIR, image + ".vxbin"))

    def upload(self, a):
        b = self.d.upload_bytes(np.ascontiguousarray(a).tobytes())
        assert b.address + b.size < 2 ** 32
        return b

    def run(self, mode, rec, scene=None):
        """rec uint32[n, REC[mode]] -> uint32[n, OUT[mode]]; scene: (nodes, nodes4 + halves,
        tris, geom buffers, num_nodes, num_nodes4, num_geom, flags)"""
        rec = np.ascontiguousarray(rec, np.uint32)
        n = rec.shape[0]
        assert rec.shape[1] == REC[mode] and n <= 4096
        words = n * OUT[mode]
        rb = self.upload(rec)
        ob = self.upload(np.full(words + GUARD, FILL, np.uint32))
        sc = scene or (None, None, None, None, 0, 0, 0, 0)
        addr = [b.address if b is not None else 0 for b in sc[:4]]
        ab = self.d.upload_bytes(struct.pack("<2I6Q4I", mode, n, rb.address, ob.address, *addr, *sc[4:]))
        try:
            self.d.start(self.k, ab)
            self.d.ready_wait()
            out = np.frombuffer(ob.read(), np.uint32)
        finally:
            for b in (rb, ob, ab):
                b.free()
        assert np.all(out[words:] == FILL), "the guard words behind the output were written"
        return out[:words].reshape(n, OUT[mode]).copy()

    def close(self):
        self.d.close()


@pytest.fixture()
def kat():
    k = Kat()
    yield k
    k.close()


def chunks(n, m=4096):
    return [slice(i, min(i + m, n)) for i in range(0, n, m)]


def mt_records(o, d, v0, e1, e2, tmin):
    r = np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in (o, d, v0, e1, e2)] +
                       [np.asarray(tmin, np.float32).reshape(-1, 1)], 1)
    return bits(r)


def test_gpu_mt_equals_oracle(oracle_lib, kat):
    """mt_hit and mt_hit_bf: verdict and t bits the oracle's on the known answers, the lattice
    table (where the oracle is the exact model, tests/test_ray_kat_cpu.py) and the general table
    with its inf, NaN, denormal and 1e30 records"""
    o, d, tri, e1, e2, tmin = ka.mt_kat_arrays()
    tables = [(o, d, tri, e1, e2, tmin), ka.mt_lattice_table(), ka.mt_general_table()]
    for tab in tables:
        hit, t = oracle_lib.mt(*tab)
        rec = mt_records(*tab)
        out = np.concatenate([kat.run(MT, rec[s]) for s in chunks(len(rec))])
        assert np.array_equal(out[:, 0], hit) and np.array_equal(out[:, 2], hit)
        assert np.array_equal(out[:, 1], bits(t)) and np.array_equal(out[:, 3], bits(t))
        print(f"mt table of {len(rec)}: {int(out[:, 0].sum())} hits on the device")
    hit, _ = oracle_lib.mt(*tables[0])
    assert [bool(h) for h in hit] == [r[4] for r in ka.MT_KAT]


def test_gpu_slab_equals_oracle(oracle_lib, kat):
    """slab and slab_nf after ray_setup: verdict, tnear and tfar bits the oracle's, over fp32
    planes and over the binary16 planes of a node record (outward rounded: +-inf past 65504)"""
    o, d, pl, tmin, tmax, _ = ka.slab_table()
    hb, hpl = ka.half_planes_outward(pl)
    # the known answers in front: fp32 rows with their planes' binary16 forms, binary16 rows with
    # the planes those decode to
    rows = ka.SLAB_KAT + ka.SLAB_HALF_KAT
    ko = np.array([r[0] for r in rows], np.float32)
    kd = np.array([r[1] for r in rows], np.float32)
    kpl = np.array([r[2] for r in ka.SLAB_KAT] + [ka.half_to_f32(r[2]) for r in ka.SLAB_HALF_KAT], np.float32)
    khb, khpl = ka.half_planes_outward(kpl)
    ktmin, ktmax = np.array([r[3] for r in rows], np.float32), np.array([r[4] for r in rows], np.float32)
    nk = len(rows)
    o, d, pl = np.concatenate([ko, o])[:4096], np.concatenate([kd, d])[:4096], np.concatenate([kpl, pl])[:4096]
    hb, hpl = np.concatenate([khb, hb])[:4096], np.concatenate([khpl, hpl])[:4096]
    tmin, tmax = np.concatenate([ktmin, tmin])[:4096], np.concatenate([ktmax, tmax])[:4096]
    rec = np.zeros((len(o), 20), np.uint32)
    rec[:, 0:3], rec[:, 3:6], rec[:, 6:12] = bits(o), bits(d), bits(pl)
    rec[:, 12], rec[:, 13], rec[:, 14:17] = bits(tmin), bits(tmax), hb
    out = kat.run(SLAB, rec)
    print(f"slab table of {len(rec)}: {int((out[:, 0] == 3).sum())} fp32 / {int((out[:, 4] == 3).sum())} binary16 boxes met")
    for k, planes in enumerate((pl, hpl)):
        hit, tn, tf = oracle_lib.slab(o, d, planes, tmin, tmax)
        assert np.array_equal(out[:, 4 * k], hit.astype(np.uint32) * 3)      # slab and slab_nf agree
        assert np.array_equal(out[:, 4 * k + 1], bits(tn)) and np.array_equal(out[:, 4 * k + 2], bits(tn))
        assert np.array_equal(out[:, 4 * k + 3], bits(tf))
    for i, r in enumerate(rows):
        k = 0 if i < len(ka.SLAB_KAT) else 1
        assert (int(out[i, 4 * k]) == 3) == r[5]
        assert out[i, 4 * k + 1] == bits([r[6]])[0] and out[i, 4 * k + 3] == bits([r[7]])[0], i
    assert nk == len(ka.SLAB_KAT) + len(ka.SLAB_HALF_KAT) and np.isinf(hpl).any()


def test_gpu_pcg_and_sampler_equal_oracle(oracle_lib, kat):
    """pcg_hash, pt_key, pt_u11, bounce_dir and tri_normal, bit for bit the oracle's"""
    po = oracle_lib
    n = 4096
    v = ka.pcg_inputs(n)
    kk = ka.pt_key_inputs()
    kk = kk[np.arange(n) % len(kk)]
    normals, keys, cls = ka.bounce_table()
    _, dd, _, e1, e2, _ = ka.mt_general_table()
    fin = np.isfinite(e1).all(1) & np.isfinite(e2).all(1) & np.isfinite(dd).all(1) & \
        (np.abs(e1).max(1) < 1e20) & (np.abs(e2).max(1) < 1e20) & (np.abs(e1).min(1) > 1e-30)
    e1, e2, dd = (np.where(fin[:, None], x, np.float32(1.0) + np.arange(3, dtype=np.float32) * (j + 1))
                  for j, x in enumerate((e1, e2, dd)))
    rec = np.zeros((n, 20), np.uint32)
    rec[:, 0], rec[:, 1:4], rec[:, 4], rec[:, 5] = v, kk, v, keys
    rec[:, 6:9], rec[:, 9:12], rec[:, 12:15], rec[:, 15:18] = bits(normals), bits(e1), bits(e2), bits(dd)
    out = kat.run(PT, rec)
    assert np.array_equal(out[:, 0], po.pcg_hash(v))
    assert np.array_equal(out[:, 1], po.pt_key(kk[:, 0], kk[:, 1], kk[:, 2]))
    assert np.array_equal(out[:, 2], bits(po.pt_u11(v)))
    want = po.pt_bounce_dir(normals, keys)
    assert np.array_equal(out[:, 3:6], bits(want))
    assert np.array_equal(out[cls == 0, 3:6].view(np.float32), normals[cls == 0])    # the pole
    assert np.array_equal(out[:, 6:9], bits(po.pt_normal(e1, e2, dd)))
    for vv, want in ka.PCG_KAT:
        assert int(out[list(v).index(vv), 0]) == want


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("ray_kat_gpu")


def device_lbvh_tree(case, po):
    """the tree the device builds (kernels/bvh_build.hip) as the renderer exports it"""
    s = rt.Scene.load(case["path"])
    r = rt.Renderer(s)
    try:
        st = r.build_bvh("lbvh")
        nodes, tris = r.export_bvh()
        n4, h4 = r.export_bvh4(), r.export_bvh4h()
    finally:
        r.close()
        s.close()
    assert st["stack4"] <= 32 and st["depth"] <= 32
    return nodes, tris, n4, h4, st["stack4"]


@pytest.mark.parametrize("name", ka.WALK_SCENES)
def test_gpu_walks_equal_brute_force_and_oracle(oracle_lib, scene_dir, name):
    po = oracle_lib
    case = ka.walk_case(name, scene_dir, po, rt)
    trees = dict(case["trees"])
    if name == "soup":
        trees["device_lbvh"] = device_lbvh_tree(case, po)
    r, skip, tie = case["rays"], case["skip"], case["tie"]
    n = len(r)
    # the oracle's brute force under the three pairs of limits the walk forms take
    zero, inf = np.zeros(n, np.float32), np.full(n, np.inf, np.float32)
    bp, bt, bo = po.trace_rays(case["tri9"], r, skip, tie)
    r_coop = np.concatenate([r[:, :6], zero[:, None], inf[:, None]], 1)
    cp, ct, _ = po.trace_rays(case["tri9"], r_coop, skip, tie)
    r_pk = np.concatenate([r[:, :6], zero[:, None], r[:, 7:8]], 1)
    _, _, ko = po.trace_rays(case["tri9"], r_pk, skip, tie)
    want = np.full((n, 12), FILL, np.uint32)
    want[:, 0] = want[:, 6] = bp.view(np.uint32)
    want[:, 1] = want[:, 7] = bits(bt)
    want[:, 2] = want[:, 8] = bo
    want[:, 3] = want[:, 11] = ko
    want[:, 4] = want[:, 9] = cp.view(np.uint32)
    want[:, 5] = want[:, 10] = bits(ct)
    launches = 0
    for image in ("rt_kat", "rt_kat_pt"):
        kat = Kat(image)
        try:
            geom = kat.upload(case["geom"])
            for tname, (nodes, tris, n4, h4, stack4) in trees.items():
                assert stack4 <= 32
                if stack4 > kat.stack:
                    continue                     # (the chain scene's trees need the deep stack)
                nb = kat.upload(nodes)
                n4b = kat.upload(np.concatenate([bits(n4).reshape(-1),
                                                 np.ascontiguousarray(h4).view(np.uint32).reshape(-1)]))
                tb = kat.upload(np.concatenate([np.ascontiguousarray(tris, np.float32), np.zeros((3, 12), np.float32)]))
                layouts = (0, RT_FLAG_BVH4, RT_FLAG_BVH4 | RT_FLAG_BVH4H) if image == "rt_kat" else \
                    (RT_FLAG_BVH4 | RT_FLAG_BVH4H,)
                for flags in layouts:
                    scene = (nb, n4b, tb, geom, len(nodes), len(n4), len(case["geom"]), flags)
                    for pat in ka.PATTERNS:
                        act = ka.activity(pat, n)
                        rec = np.zeros((n, 12), np.uint32)
                        rec[:, 0:8] = bits(r)
                        rec[:, 8] = skip.view(np.uint32)
                        rec[:, 9] = tie.astype(np.uint32) | (act.astype(np.uint32) << 1)
                        out = kat.run(WALK, rec, scene)
                        launches += 1
                        exp = want.copy()
                        exp[~act] = FILL
                        if not flags & RT_FLAG_BVH4H:
                            exp[:, 3:6] = FILL       # no packet / pair walk over these layouts
                        bad = np.argwhere(out != exp)
                        assert len(bad) == 0, (name, image, tname, hex(flags), pat, len(bad), bad[:8].tolist(),
                                               out[bad[0][0]].tolist(), exp[bad[0][0]].tolist())
                for b in (nb, n4b, tb):
                    b.free()
        finally:
            kat.close()
    print(f"{name}: {launches} launches of {n} rays over {len(trees)} trees; closest hits {int((bp >= 0).sum())}, "
          f"occluded {int(bo.sum())}, pair-walk hits {int((cp >= 0).sum())}, packet occluded {int(ko.sum())}")
