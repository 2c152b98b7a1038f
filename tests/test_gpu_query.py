"""GPU tests of caller-supplied rays (vx_rt.h rt_query_reserve / rt_query_trace /
rt_query_keys; images rt_query -- kernels/rt_query_kernel.hip -- and
rt_query_keys, kernels/rt_query_keys_kernel.hip) through Renderer.trace_rays.

Closest hits are held bit for bit to the exact rational model of the lattice
scenes (tests/ray_reference.py) and to the oracle's brute force
(orc_trace_rays); any-hit verdicts to the oracle's, every returned occluder to
the model; the deep-stack image to brute force on the chain scene; tekkaman's
eye and ambient-occlusion rays to brute force and to the device's own ao()
counts.  Then the launch shapes, the permutation, the keys, malformed rays,
stream order against frames, every refusal, and the tensor path.  No reference
exists for this entry point."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ao_reference as ar  # noqa: E402
import query_reference as qr  # noqa: E402
import ray_known_answers as ka  # noqa: E402
import ray_reference as rr  # noqa: E402
import rt_model_checks as mc  # noqa: E402
from test_ao_cpu import SEEDS, oracle_records  # noqa: E402

pytestmark = pytest.mark.gpu

from skybox_rt_amd import rt  # noqa: E402

INF = float("inf")
N = ka.N_RAYS
LATTICE = tuple(ka.LATTICE_SCENES)
_state = {}


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("query_gpu")


def bits(a):
    return qr.bits(a)


def walk(name, scene_dir, po):
    """-> (case, renderer): the walk scene loaded from its trace, the default device tree, a small
    frame configured and N rays reserved -- once per process"""
    if name not in _state:
        case = ka.walk_case(name, scene_dir, po, rt)
        s = rt.Scene.load(case["path"])
        r = rt.Renderer(s)
        r.configure(32, 32, shadows=False)
        r.query_reserve(N)
        _state[name] = (case, r, s)
    return _state[name][:2]


def brute(case, po, use_skip=True):
    """the oracle's brute force over the scene's triangles, tie_high false -> (pid, t, occluded); cached"""
    key = ("brute", use_skip)
    if key not in case:
        skip = case["skip"] if use_skip else np.full(N, -1, np.int32)
        case[key] = po.trace_rays(case["tri9"], case["rays"], skip, np.zeros(N, np.uint8))
    return case[key]


def same_hits(got, want_pid, want_t, what=""):
    pid, t = got
    assert pid.dtype == np.int32 and t.dtype == np.float32 and pid.shape == t.shape == want_pid.shape
    bad = np.flatnonzero((pid != want_pid) | (bits(t) != bits(want_t)))
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), pid[bad[:4]].tolist(), np.asarray(want_pid)[bad[:4]].tolist(),
                           t[bad[:4]].tolist(), np.asarray(want_t)[bad[:4]].tolist())


def raw_hits(r, n=N):
    return r.query_hits(n)


def raw_keys(r, n=N):
    out = np.zeros(n, np.uint32)
    rt._check(rt.lib().rt_query_read_keys(r._h, out.ctypes.data, 0, n), "rt_query_read_keys")
    return out


def refused(fn, *a, match="", **kw):
    with pytest.raises(rt.RtError) as e:
        fn(*a, **kw)
    assert "(-2)" in str(e.value) and match in str(e.value), str(e.value)


# ---- closest and any against the references --------------------------------------------------

@pytest.mark.parametrize("name", LATTICE)
def test_closest_equals_model_and_oracle(po, scene_dir, name):
    case, r = walk(name, scene_dir, po)
    lat, rays = case["lat"], case["rays"]
    box = r.query_buffers()["box"]
    s = rt.Scene.load(case["path"])
    assert np.array_equal(box, qr.corner_box(s.prims()[:, :, [0, 1, 3]]))
    s.close()
    for use_skip in (True, False):
        skip = case["skip"] if use_skip else None
        mskip = case["skip"] if use_skip else np.full(N, -1, np.int32)
        mp, mt, _ = rr.closest_hits(lat["inside"], lat["t"], rays[:, 6], rays[:, 7], mskip, np.zeros(N, bool))
        bp, bt, _ = brute(case, po, use_skip)
        assert np.array_equal(mp, bp) and np.array_equal(bits(mt), bits(bt))   # the references agree
        got = r.trace_rays(rays, "closest", skip=skip)
        assert len(got[0]) == N                                                 # no ray is left out
        same_hits(got, mp, mt, (name, "model", use_skip))
        same_hits(got, bp, bt, (name, "oracle", use_skip))
        print(f"{name} skip={use_skip}: {int((got[0] >= 0).sum())} of {N} rays hit")
        assert (got[0] >= 0).sum() > N // 8 and (got[0] < 0).sum() > N // 16


@pytest.mark.parametrize("name", LATTICE)
def test_any_equals_oracle_and_names_a_met_triangle(po, scene_dir, name):
    case, r = walk(name, scene_dir, po)
    lat, rays = case["lat"], case["rays"]
    for use_skip in (True, False):
        skip = case["skip"] if use_skip else None
        mskip = case["skip"] if use_skip else np.full(N, -1, np.int32)
        _, _, occ = brute(case, po, use_skip)
        pid, t = r.trace_rays(rays, "any", skip=skip)
        assert np.array_equal(pid >= 0, occ.astype(bool)), (name, int(((pid >= 0) != occ.astype(bool)).sum()))
        h = np.flatnonzero(pid >= 0)
        p = pid[h]
        assert (p < len(case["tri9"])).all() and (p != mskip[h]).all()
        assert lat["inside"][h, p].all()                                        # the model says the ray meets it
        assert np.array_equal(bits(t[h]), bits(lat["t"][h, p]))                 # at mt_hit's t
        assert (t[h] > rays[h, 6]).all() and (t[h] < rays[h, 7]).all()          # inside the limits
        assert not t[pid < 0].any()
        print(f"{name} skip={use_skip}: {len(h)} of {N} rays occluded")
        assert len(h) > N // 8


def test_chain_scene_on_the_deep_stack(po, scene_dir):
    case, r = walk("chain", scene_dir, po)
    assert case["trees"]["sah"][4] == 32          # the tree's BVH4 stack need: the deep image's bound
    for use_skip in (True, False):
        skip = case["skip"] if use_skip else None
        bp, bt, bo = brute(case, po, use_skip)
        same_hits(r.trace_rays(case["rays"], "closest", skip=skip), bp, bt, ("chain", use_skip))
        pid, t = r.trace_rays(case["rays"], "any", skip=skip)
        assert np.array_equal(pid >= 0, bo.astype(bool))
    assert (bp >= 0).sum() > N // 8


# ---- tekkaman: eye rays and ambient-occlusion rays --------------------------------------------

def tekkaman(po):
    """64 x 64 tekkaman: the renderer, and 4096 rays -- the one ambient-occlusion ray (sample SEEDS[0],
    unbounded) of each of the frame's ray pixels (the frame has 417: every one there is), and eye rays
    through pixel centres for the rest of the table, in pixel order"""
    if "tekkaman" not in _state:
        W = H = 64
        sc, pid, t = oracle_records("tekkaman", W, H)
        gid, of_pid, tri9 = ar.geometry(sc)
        v, fv, dirs = ar.verdicts(sc, W, H, SEEDS[0], INF, 1, pid, t, with_rays=True)
        na = len(fv["idx"])
        rays = np.zeros((W * H, 8), np.float32)
        skip = np.full(W * H, -1, np.int32)          # geometry indices (the oracle's); gid maps them to pids
        rays[:na, 0:3], rays[:na, 3:6], rays[:na, 7] = fv["P"], dirs[0], INF
        skip[:na] = fv["tri"]
        pix = np.arange(W * H - na)
        x, y = (pix % W).astype(np.float32), (pix // W).astype(np.float32)
        sx, sy = np.float32(2.0) / np.float32(W), np.float32(2.0) / np.float32(H)
        rays[na:, 3] = ((x + np.float32(0.5)).astype(np.float64) * np.float64(sx) - 1.0).astype(np.float32)
        rays[na:, 4] = ((y + np.float32(0.5)).astype(np.float64) * np.float64(sy) - 1.0).astype(np.float32)
        rays[na:, 5], rays[na:, 7] = 1.0, INF
        s = rt.Scene.load(mc.scene_file("tekkaman"))
        r = rt.Renderer(s)
        r.configure(W, H)
        r.query_reserve(W * H)
        dskip = np.where(skip >= 0, gid[np.maximum(skip, 0)], -1).astype(np.int32)
        _state["tekkaman"] = dict(r=r, s=s, rays=rays, skip=skip, dskip=dskip, gid=gid, tri9=tri9, fv=fv, v=v, na=na)
    return _state["tekkaman"]


def test_tekkaman_closest_equals_brute_force(po):
    k = tekkaman(po)
    n = len(k["rays"])
    assert n == 4096 and n - k["na"] >= n // 2
    bp, bt, _ = po.trace_rays(k["tri9"], k["rays"], k["skip"], np.zeros(n, np.uint8))
    want = np.where(bp >= 0, k["gid"][np.maximum(bp, 0)], -1).astype(np.int32)
    got = k["r"].trace_rays(k["rays"], "closest", skip=k["dskip"])
    same_hits(got, want, bt, "tekkaman")
    print(f"tekkaman: {int((want[:k['na']] >= 0).sum())} of {k['na']} AO rays and "
          f"{int((want[k['na']:] >= 0).sum())} of {n - k['na']} eye rays hit")
    assert (want[k["na"]:] >= 0).sum() > 200 and (want[:k["na"]] >= 0).sum() > 20


def test_tekkaman_any_hit_counts_equal_ao(po):
    k = tekkaman(po)
    r, na, fv = k["r"], k["na"], k["fv"]
    pid, _ = r.trace_rays(k["rays"], "any", skip=k["dskip"])
    W = H = 64
    occ = np.zeros(W * H, np.uint32)
    occ[fv["idx"]] = pid[:na] >= 0
    assert np.array_equal(occ.reshape(H, W), k["v"][0].astype(np.uint32))      # the composition's verdicts
    r.aov()
    r.ao_begin(radius=INF, seed=SEEDS[0])
    r.ao(1)
    counts = r.ao_records()
    assert np.array_equal(occ.reshape(H, W), counts), int((occ.reshape(H, W) != counts).sum())
    assert counts.sum() > 20


# ---- launch shapes, buffers, stream order -----------------------------------------------------

def test_launch_shapes_and_stores_past_n(po, scene_dir):
    case, r = walk("soup", scene_dir, po)
    rays, skip = case["rays"], case["skip"]
    full = r.trace_rays(rays, "closest", skip=skip)
    other = r.trace_rays(rays[::-1].copy(), "closest", skip=skip[::-1].copy())
    assert (other[0] != full[0]).sum() > N // 4
    for n in (1, 63, 64, 65, 4095):
        r.trace_rays(rays[::-1].copy(), "closest", skip=skip[::-1].copy())      # the earlier launch's values
        got = r.trace_rays(rays[:n], "closest", skip=skip[:n])
        same_hits(got, full[0][:n], full[1][:n], n)
        after = raw_hits(r)
        same_hits((after[0][:n], after[1][:n]), full[0][:n], full[1][:n], n)
        same_hits((after[0][n:], after[1][n:]), other[0][n:], other[1][n:], ("past n", n))


def test_permutations(po, scene_dir):
    case, r = walk("soup", scene_dir, po)
    rays, skip = case["rays"], case["skip"]
    h = rt.lib()
    rng = np.random.default_rng(5)
    for mode in ("closest", "any"):
        for n in (N, 4095):
            plain = r.trace_rays(rays[:n], mode, skip=skip[:n])
            keys = r.query_keys(rays[:n])
            perms = {"identity": np.arange(n), "random": rng.permutation(n), "keys": np.argsort(keys, kind="stable")}
            for what, perm in perms.items():
                r.trace_rays(rays[:n][::-1].copy(), mode, skip=skip[:n][::-1].copy())   # other hits in the buffer
                r._query_upload("test", rays[:n], skip[:n])
                p32 = np.ascontiguousarray(perm, np.uint32)
                rt._check(h.rt_query_write_perm(r._h, p32.ctypes.data, 0, n), "rt_query_write_perm")
                rt._check(h.rt_query_trace(r._h, n, rt.QUERY_MODES[mode], rt.RT_QUERY_SKIP | rt.RT_QUERY_PERM),
                          "rt_query_trace")
                same_hits(raw_hits(r, n), plain[0], plain[1], (mode, n, what))
            same_hits(r.trace_rays(rays[:n], mode, skip=skip[:n], sort=True), plain[0], plain[1], (mode, n, "sort"))


def test_permutation_entries_out_of_range_are_dropped(po, scene_dir):
    case, r = walk("soup", scene_dir, po)
    rays = case["rays"]
    n = 130
    plain = r.trace_rays(rays[:n], "closest")
    before = raw_hits(r)
    perm = np.arange(n, dtype=np.uint32)
    perm[[3, 64, 129]] = (n, 0x7FFFFFFF, 0xFFFFFFFF)
    rt._check(rt.lib().rt_query_write_perm(r._h, perm.ctypes.data, 0, n), "rt_query_write_perm")
    r.trace_rays(rays[:n][::-1].copy(), "closest")                              # other hits for 3, 64, 129
    other = raw_hits(r)
    r._query_upload("test", rays[:n], None)
    rt._check(rt.lib().rt_query_trace(r._h, n, 0, rt.RT_QUERY_PERM), "rt_query_trace")
    got = raw_hits(r)
    keep = np.ones(N, bool)
    keep[[3, 64, 129]] = False
    same_hits((got[0][:n][keep[:n]], got[1][:n][keep[:n]]), plain[0][keep[:n]], plain[1][keep[:n]], "in range")
    same_hits((got[0][~keep], got[1][~keep]), other[0][~keep], other[1][~keep], "dropped slots")
    same_hits((got[0][n:], got[1][n:]), before[0][n:], before[1][n:], "past n")


@pytest.mark.parametrize("name", ka.WALK_SCENES)
def test_device_keys_equal_host_keys(po, scene_dir, name):
    case, r = walk(name, scene_dir, po)
    box = r.query_buffers()["box"]
    hand, _, _ = qr.hand_rays()
    table = np.concatenate([case["rays"][:N - len(hand)], hand])
    want = rt.query_key(table, box)
    assert np.array_equal(want, qr.key_numpy(table, box))
    got = r.query_keys(table)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (name, len(bad), table[bad[0]].tolist(), hex(int(got[bad[0]])), hex(int(want[bad[0]])))
    assert (got[-7:] == qr.MISS_KEY).all()
    # the words behind n keep the earlier launch's keys
    for n in (1, 63, 65):
        r.query_keys(table)
        first = r.query_keys(table[::-1][:n].copy())
        assert np.array_equal(first, want[::-1][:n])
        assert np.array_equal(raw_keys(r)[n:], want[n:])


@pytest.mark.parametrize("kind", sorted(qr.MALFORMED_KINDS))
@pytest.mark.parametrize("mode", ["closest", "any"])
def test_malformed_rays_miss_and_leave_their_wave_alone(po, scene_dir, kind, mode):
    case, r = walk("soup", scene_dir, po)
    rays, skip = case["rays"][:128], case["skip"][:128]
    plain = r.trace_rays(rays, mode, skip=skip)
    assert (plain[0][:64] >= 0).sum() > 8
    bad = qr.with_malformed(rays, kind)
    assert list(np.flatnonzero(qr.malformed(bad))) == [0, 31, 63]
    pid, t = r.trace_rays(bad, mode, skip=skip)
    m = np.zeros(128, bool)
    m[[0, 31, 63]] = True
    assert (pid[m] == -1).all() and not bits(t[m]).any()
    same_hits((pid[~m], t[~m]), plain[0][~m], plain[1][~m], (kind, mode))
    # sorted, they go to the end together and the hits stay at the rays' own indices
    spid, st = r.trace_rays(bad, mode, skip=skip, sort=True)
    same_hits((spid, st), pid, t, (kind, mode, "sort"))


def test_tmax_infinity_is_admitted(po, scene_dir):
    case, r = walk("soup", scene_dir, po)
    rays = case["rays"].copy()
    rays[:, 6], rays[:, 7] = 0.0, INF
    bp, bt, _ = po.trace_rays(case["tri9"], rays, np.full(N, -1, np.int32), np.zeros(N, np.uint8))
    same_hits(r.trace_rays(rays, "closest"), bp, bt, "tmax inf")


def test_stream_order_and_isolation(po):
    k = tekkaman(po)
    W = H = 64
    s = rt.Scene.load(mc.scene_file("tekkaman"))
    ref = rt.Renderer(s)                          # a renderer that never runs a query
    ref.configure(W, H)
    ref.render()
    want_fb = ref.framebuffer()
    ref.close()
    r = rt.Renderer(s)
    r.configure(W, H)
    r.query_reserve(W * H)
    sync = r.trace_rays(k["rays"], "closest", skip=k["dskip"])
    r.trace_rays(k["rays"][::-1].copy(), "closest")                             # other hits in the buffer
    r.render()
    fb1 = r.framebuffer()
    assert r.trace_rays(k["rays"], "closest", skip=k["dskip"], wait=False) is None
    r.start()
    r.wait()
    fb2 = r.framebuffer()
    hits = r.query_hits(W * H)
    assert np.array_equal(fb1, want_fb) and np.array_equal(fb2, want_fb)
    same_hits(hits, sync[0], sync[1], "asynchronous")
    # the reserve survives a configure to another size, set_light and set_lights
    r.configure(40, 24)
    r.set_light((10.0, 20.0, 30.0))
    same_hits(r.trace_rays(k["rays"], "closest", skip=k["dskip"]), sync[0], sync[1], "after configure")
    r.set_lights([(0.0, 60.0, 80.0), (40.0, 10.0, 60.0)])
    same_hits(r.trace_rays(k["rays"], "closest", skip=k["dskip"]), sync[0], sync[1], "after set_lights")
    # a path-frame configuration admits queries, and its frames are what they are without one
    r.configure(W, H, path=True, bounces=1)
    r.render()
    p1 = r.framebuffer()
    same_hits(r.trace_rays(k["rays"], "closest", skip=k["dskip"]), sync[0], sync[1], "path frame")
    r.render()
    assert np.array_equal(r.framebuffer(), p1)
    r.close()
    s.close()


def test_scene_without_geometry_answers_misses(po):
    from conftest import scene_path
    s = rt.Scene.load(scene_path("triangle"))      # one drawcall, not depth-tested: a screen layer
    assert s.info()["num_geometry"] == 0 and s.info()["num_prims"] > 0
    r = rt.Renderer(s)
    r.configure(32, 32, shadows=False)
    r.query_reserve(256)
    rays = np.zeros((200, 8), np.float32)
    rays[:, 5], rays[:, 7] = 1.0, INF
    for mode in ("closest", "any"):
        pid, t = r.trace_rays(rays, mode)
        assert (pid == -1).all() and not bits(t).any()
    assert not r.query_buffers()["box"].any()
    r.close()
    s.close()


def test_refusals(po, scene_dir):
    case, _ = walk("soup", scene_dir, po)
    s = rt.Scene.load(case["path"])
    r = rt.Renderer(s)
    h = rt.lib()
    rays = case["rays"]
    refused(r.query_reserve, 64, match="not configured")
    r.configure(32, 32, shadows=False)
    refused(r.trace_rays, rays[:8], match="no reserve")
    refused(r.query_keys, rays[:8], match="no reserve")
    refused(r.query_buffers, match="no reserve")
    refused(r.query_hits, 8, match="no reserve")
    refused(r.query_reserve, 0, match="max_rays")
    refused(r.query_reserve, (1 << 24) + 1, match="max_rays")
    r.query_reserve(1 << 22)                      # 2^22 rays are admitted
    assert r.query_buffers()["capacity"] == 1 << 22
    r.query_reserve(64)
    assert r.query_buffers()["capacity"] == 64
    refused(r.trace_rays, rays[:65], match="capacity")
    refused(r.query_keys, rays[:65], match="capacity")
    r.trace_rays(rays[:64])

    def call(fn, *a):
        rt._check(fn(r._h, *a), fn.__name__)

    refused(call, h.rt_query_trace, 0, 0, 0, match="n is 0")
    refused(call, h.rt_query_keys, 0, match="n is 0")
    refused(call, h.rt_query_trace, 8, 2, 0, match="unknown mode")
    refused(call, h.rt_query_trace, 8, 0, 4, match="unknown flag")
    refused(call, h.rt_query_write_rays, rays.ctypes.data, 60, 8, match="capacity")
    refused(call, h.rt_query_read_hits, rays.ctypes.data, 1, 64, match="capacity")
    # launches started and not waited for: the reserve stays
    r.trace_rays(rays[:64], wait=False)
    refused(r.query_reserve, 128, match="not waited for")
    r.wait()
    r.query_reserve(128)
    # a tree of another layout
    r.configure(32, 32, shadows=False, bvh_width=2)
    refused(r.trace_rays, rays[:8], match="binary16 BVH4")
    r.configure(32, 32, shadows=False)
    same_hits(r.trace_rays(rays[:128]), *r.trace_rays(rays[:128]))
    r.close()
    s.close()


def test_torch_tensors_stay_on_the_device(po, scene_dir):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch.cuda is unavailable")
    case, r = walk("soup", scene_dir, po)
    rays, skip = case["rays"], case["skip"]
    tr, ts = torch.from_numpy(rays).cuda(), torch.from_numpy(skip).cuda()
    for mode in ("closest", "any"):
        for sort in (False, True):
            want = r.trace_rays(rays, mode, skip=skip)
            r.trace_rays(rays[::-1].copy(), mode)
            pid, t = r.trace_rays(tr, mode, skip=ts, sort=sort)
            assert pid.is_cuda and t.is_cuda and pid.dtype == torch.int32 and t.dtype == torch.float32
            same_hits((pid.cpu().numpy(), t.cpu().numpy()), want[0], want[1], (mode, sort))
    keys = r.query_keys(tr)
    assert keys.is_cuda and np.array_equal(keys.cpu().numpy().astype(np.uint32), r.query_keys(rays))
    refused_msg = None
    try:
        r.trace_rays(tr.double())
    except rt.RtError as e:
        refused_msg = str(e)
    assert refused_msg and "float32" in refused_msg
