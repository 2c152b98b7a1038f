"""What tests/test_rt_model_cpu.py and tests/test_gpu_rt_model.py share: the
scenes, the model's moments (computed once per process), the criteria that hold
a set of frames to the model (tests/rt_reference.py), their constants, and
check_sensitivity(), which shows on the model alone that the criteria notice
each documented part of the estimator going missing.  TEST INFRASTRUCTURE ONLY.

`python tests/rt_model_checks.py calibrate` runs the model against itself
(two independent generator streams, REPS repetitions) and prints the worst
statistic of each kind; the constants below are those figures times 1.5
(DESIGN 5 records both).  Nothing here was tuned on the oracle or the device.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

import rt_reference as rr
import synth_scene
from conftest import scene_path

N_FRAMES = 2048            # frames of consecutive seeds taken from the code under test
M_SAMPLES = 4096           # the model's samples per pixel
SEED0 = 1000               # the first of the consecutive seeds
MODEL_STREAM = 20261       # numpy Generator seed of the model's samples
BOUNCES = (1, 4)
LIGHT = (0.0, 60.0, 80.0)
PATH_LIGHTS = [(0.0, 60.0, 80.0), (30.0, -20.0, 95.0)]
TEKKAMAN_LIGHTS = [(0.0, 60.0, 80.0), (40.0, 10.0, 60.0), (-30.0, -20.0, 90.0)]
AMBIGUOUS_CAP = 0.01       # share of a case's shadow rays the model may leave undecided

# --- measured, model against model (calibrate(); DESIGN 5 has the table) -----------
# Over 20 repetitions x 2 bounce depths, 996 channels each: the worst per-channel |z|
# was 10.75 (a channel whose rare bright path the M samples met too seldom for a
# variance; the next were 6.22, 5.44, 5.03 and 35 repetitions stayed under 5), the
# worst pooled |z| 3.57, variance ratio 3.45, lag-1 autocorrelation 2.05, neighbour
# correlation 3.19 (the sampling errors are the Gaussian ones; channels of a pixel
# share a path and sample values are skewed, so these run past 3).  Each x 1.5:
Z_CHANNEL = 16.2           # a single channel's mean
Z_POOLED = 5.4             # a single statistic of the whole image (the worst of the four, 3.57)
# a channel's variance estimate is floored at the variance of rounding to 8 bits:
# a rare event that none of the model's M samples met leaves it 0 otherwise
VAR_FLOOR = 1.0 / 12.0

REPS = 20

_dir = None
_cache = {}


def scene_file(name):
    """path of a scene by name: one of tests/golden/scenes, or a synthetic one
    written once per process into a temporary directory"""
    global _dir
    makers = {"interreflection": synth_scene.make_interreflection_scene,
              "convex": synth_scene.make_convex_scene,
              "shadow_edge": synth_scene.make_shadow_edge_scene}
    if name not in makers:
        return scene_path(name)
    if _dir is None:
        _dir = tempfile.TemporaryDirectory(prefix="rt_model_")
    p = os.path.join(_dir.name, name + ".cgltrace.gz")
    if not os.path.exists(p):
        makers[name](p)
    return p


def model(name, w, h):
    """(cgltrace scene, Model) of a scene at a size"""
    from oracle import cgltrace
    if ("scene", name) not in _cache:
        _cache[("scene", name)] = cgltrace.load(scene_file(name))
    sc = _cache[("scene", name)]
    if ("model", name, w, h) not in _cache:
        _cache[("model", name, w, h)] = rr.Model(sc.prim_verts, sc.drawcalls, w, h)
    return sc, _cache[("model", name, w, h)]


def rgb(frame):
    """uint32 ARGB [...] -> int64 [..., 3]"""
    f = np.asarray(frame, np.uint32)
    return np.stack([(f >> 16) & 0xFF, (f >> 8) & 0xFF, f & 0xFF], -1).astype(np.int64)


# ---- shadow verdicts and the plane parameter ---------------------------------------

def verdict(name, w, h, pid, light):
    key = ("verdict", name, w, h, tuple(light))
    if key not in _cache:
        _cache[key] = model(name, w, h)[1].shadow_verdict(pid, light)
    return _cache[key]


def check_verdicts(v, rays, occluded, t, known=None, what=""):
    """Holds one light's verdicts (bool [H, W]), the shadow-ray pixels and the plane
    t of the code under test to the model's verdict record v.  Returns the number
    of ambiguous rays."""
    assert np.array_equal(rays, v["rays"]), f"{what}: {int((rays != v['rays']).sum())} pixels start a ray on one side only"
    n = int(v["rays"].sum())
    amb = int((v["rays"] & ~v["robust"]).sum())
    assert amb <= AMBIGUOUS_CAP * n, f"{what}: {amb} of {n} rays ambiguous"
    cmp_ = v["rays"] & v["robust"]
    if known is not None:
        cmp_ = cmp_ & known
    bad = int((np.asarray(occluded, bool) != v["occluded"])[cmp_].sum())
    assert bad == 0, f"{what}: {bad} of {int(cmp_.sum())} robust verdicts differ"
    check_plane_t(v, t, what)
    return amb


def check_plane_t(v, t, what="", pull=rr.PULL):
    """|t - t_model| <= 2^-14 |t_model| on every ray pixel, and the origin d t (1 - pull)
    stays on the eye's side of its plane by at least half the documented pull-back
    (implied by the bound: 1 - (1 + 2^-14)(1 - 2^-12) > 2^-13)"""
    r = v["rays"]
    tm = v["t"][r]
    got = np.asarray(t, np.float64)[r]
    rel = np.abs(got - tm) / np.abs(tm)
    worst = float(rel.max()) if rel.size else 0.0
    print(f"{what}: plane t worst relative error {worst:.3g} over {rel.size} rays")
    assert worst <= rr.T_BOUND, f"{what}: plane t off by {worst:.3g} relative"
    # the plane's parameter is t_model, so the origin's distance to it, as a share of
    # the eye's, is 1 - t (1 - pull) / t_model
    share = 1.0 - got * (1.0 - pull) / tm
    assert (share >= rr.PULL / 2).all(), f"{what}: origin not on the eye's side: least share {share.min():.3g}"


# ---- path frames -----------------------------------------------------------------------

def model_moments(name, w, h, pid, plain, lights, bounces, v=rr.TRUE, samples=M_SAMPLES, stream=MODEL_STREAM):
    """(idx, mean[n, 3], var[n, 3]) of the model's samples; computed once per process"""
    key = ("moments", name, w, h, tuple(np.ravel(lights)), bounces, tuple(sorted(v.items(), key=str)), samples, stream)
    if key not in _cache:
        idx, s = model(name, w, h)[1].path_samples(pid, plain, lights, bounces, samples,
                                                   np.random.default_rng(stream), v)
        _cache[key] = (idx,) + rr.moments(s)
    return _cache[key]


def check_deterministic(name, w, h, pid, plain, light, bounces, frame, what=""):
    """a frame that no random number reaches: every channel within 0.5 LSB of the
    model's unrounded value"""
    idx, s = model(name, w, h)[1].path_samples(pid, plain, light, bounces, 2, np.random.default_rng(1), unrounded=True)
    assert np.array_equal(s[0], s[1]), f"{what}: the model itself is not deterministic here"
    d = np.abs(rgb(np.asarray(frame).reshape(-1)[idx]) - s[0])
    print(f"{what}: {len(idx)} path pixels, max difference {float(d.max()) if d.size else 0:.4f} LSB")
    assert len(idx) > 0 and d.max() <= 0.5, f"{what}: {int((d > 0.5).sum())} channels more than 0.5 LSB off the model"


def channel_stats(mean_a, n_a, mean_m, var_m, m):
    """-> (per-channel z, pooled z over the stochastic channels, pooled difference, its se)"""
    se2 = np.maximum(var_m, VAR_FLOOR) * (1.0 / n_a + 1.0 / m)
    diff = mean_a - mean_m
    z = diff / np.sqrt(se2)
    st = var_m > 0
    n = int(st.sum())
    pooled = float(diff[st].sum() / n)
    pse = float(np.sqrt(se2[st].sum()) / n)
    return z, pooled / pse, pooled, pse


def check_means(mean_a, n_a, mean_m, var_m, m=M_SAMPLES, what=""):
    z, zp, pooled, pse = channel_stats(mean_a, n_a, mean_m, var_m, m)
    print(f"{what}: {z.size} channels, worst |z| {np.abs(z).max():.2f}, z sd {z[var_m > 0].std():.2f}, "
          f"pooled difference {pooled:+.4f} +- {pse:.4f} LSB (z {zp:+.2f})")
    assert np.abs(z).max() <= Z_CHANNEL, f"{what}: a channel's mean is {np.abs(z).max():.2f} se from the model's"
    assert abs(zp) <= Z_POOLED, f"{what}: pooled difference {pooled:+.4f} LSB is {zp:+.2f} se"


def independence_stats(x):
    """x float[N, n] (a value per frame and path pixel) -> the z of three statistics
    that are 0 in expectation when pixels and frames are independent:
    - the variance over frames of the image mean against sum(per-pixel variances) / n^2
      (a ratio of 1; sd sqrt(2 / (N - 1)));
    - the lag-1 autocorrelation of the image mean over consecutive frames (sd 1 / sqrt(N));
    - the mean correlation of adjacent columns of x (the caller passes horizontally
      adjacent pixel pairs as columns 2k, 2k + 1; se 1 / sqrt(N pairs))."""
    N, n = x.shape
    g = x.mean(1)
    ratio = g.var(ddof=1) / (x.var(0, ddof=1).sum() / n ** 2)
    gc = g - g.mean()
    lag1 = float((gc[:-1] * gc[1:]).sum() / (gc * gc).sum())
    return dict(ratio=(ratio, (ratio - 1.0) / np.sqrt(2.0 / (N - 1))),
                lag1=(lag1, lag1 * np.sqrt(N)))


def neighbour_stat(x, idx, w):
    """mean correlation over frames of horizontally adjacent path pixels whose values
    both vary -> (mean, z)"""
    pos = {int(p): k for k, p in enumerate(idx)}
    sd = x.std(0)
    pairs = [(k, pos[int(p) + 1]) for k, p in enumerate(idx)
             if (int(p) + 1) % w and int(p) + 1 in pos and sd[k] > 0 and sd[pos[int(p) + 1]] > 0]
    a = np.array([p[0] for p in pairs])
    b = np.array([p[1] for p in pairs])
    xc = (x - x.mean(0)) / np.where(sd > 0, sd, 1.0)
    c = (xc[:, a] * xc[:, b]).mean(0)
    return float(c.mean()), float(c.mean() * np.sqrt(len(x) * len(pairs))), len(pairs)


def check_independence(frames_rgb, idx, w, what=""):
    """frames_rgb int[N, n, 3] of the path pixels idx over consecutive seeds"""
    x = frames_rgb.astype(np.float64).mean(2)             # a pixel's channels share its path
    st = independence_stats(x)
    nb, znb, npairs = neighbour_stat(x, idx, w)
    print(f"{what}: variance ratio {st['ratio'][0]:.3f} (z {st['ratio'][1]:+.2f}), lag-1 {st['lag1'][0]:+.4f} "
          f"(z {st['lag1'][1]:+.2f}), neighbour correlation {nb:+.4f} over {npairs} pairs (z {znb:+.2f})")
    for name, z in (("variance ratio", st["ratio"][1]), ("lag-1 autocorrelation", st["lag1"][1]),
                    ("neighbour correlation", znb)):
        assert abs(z) <= Z_POOLED, f"{what}: {name} is {z:+.2f} sd from independence"
    return st, (nb, znb)


# ---- the criteria notice what they should -----------------------------------------------

PATH_VARIANTS = dict(uniform_hemisphere=dict(uniform_hemisphere=True), unfaced_normal=dict(face_normal=False),
                     no_bounce_shadows=dict(bounce_shadows=False), no_sky=dict(sky=False))
VERDICT_VARIANTS = dict(no_self_skip=dict(self_skip=False), segment_past_light=dict(segment_end=False),
                        light_independent=dict(fixed_light=(0.0, 60.0, 80.0)))


def _fails(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError:
        return True
    return False


def check_sensitivity(pid_of, plain_of):
    """pid_of(name, w, h), plain_of(name, w, h): the raster's winner and the unlit
    frame (pinned components).  Shows on the model alone that
    - a variant estimator's N_FRAMES samples fail check_means against the true
      model's M_SAMPLES moments (at one bounce depth at least);
    - samples whose bounce draws are shared by all pixels of a frame, or by consecutive
      frames, fail check_independence;
    - a variant verdict differs from the true one on robust pixels of the shadow-edge
      scene under its three lights;
    - an origin without the pull-back fails check_plane_t.
    Raises AssertionError naming the first variant the criteria let through."""
    w = h = 32
    pid, plain = pid_of("interreflection", w, h), plain_of("interreflection", w, h)
    for name, kw in PATH_VARIANTS.items():
        caught = False
        for b in BOUNCES[::-1]:
            if caught:
                break
            idx, mean_m, var_m = model_moments("interreflection", w, h, pid, plain, LIGHT, b)
            _, mean_v, _ = model_moments("interreflection", w, h, pid, plain, LIGHT, b, rr.variant(**kw),
                                         samples=N_FRAMES, stream=MODEL_STREAM + 7)
            caught |= _fails(check_means, mean_v, N_FRAMES, mean_m, var_m, what=f"variant {name}, {b} bounces")
        assert caught, f"the path criteria do not notice: {name}"
    for share in ("pixels", "seeds"):                         # draws that are not independent
        idx, s = model("interreflection", w, h)[1].path_samples(pid, plain, LIGHT, 1, N_FRAMES,
                                                                 np.random.default_rng(MODEL_STREAM + 11),
                                                                 rr.variant(shared_draws=share))
        assert _fails(check_independence, s.astype(np.int64), idx, w, what=f"variant draws shared over {share}"), \
            f"the independence criteria do not notice draws shared over {share}"
    w = h = 64
    pid = pid_of("shadow_edge", w, h)
    m = model("shadow_edge", w, h)[1]
    for name, kw in VERDICT_VARIANTS.items():
        caught = False
        for L in synth_scene.SHADOW_EDGE_LIGHTS:
            v = verdict("shadow_edge", w, h, pid, L)
            vv = m.shadow_verdict(pid, L, v=rr.variant(**kw))
            caught |= _fails(check_verdicts, v, vv["rays"], vv["occluded"], vv["t"], what=f"variant {name}")
        assert caught, f"the verdict criteria do not notice: {name}"
    v = verdict("shadow_edge", w, h, pid, synth_scene.SHADOW_EDGE_LIGHTS[0])
    assert _fails(check_plane_t, v, v["t"], "variant no pull-back", pull=0.0), "check_plane_t does not notice a missing pull-back"
    assert _fails(check_plane_t, v, v["t"] * (1 + 2.0 ** -13), "variant t off"), "check_plane_t does not notice t off by 2^-13"


# ---- calibration: the model against itself ------------------------------------------------

def calibrate(pid, plain, reps=REPS):
    """prints, per bounce depth and repetition, the statistics of N_FRAMES samples of
    one generator stream against M_SAMPLES of another, and the worst of each kind"""
    w = h = 32
    m = model("interreflection", w, h)[1]
    worst = dict(channel=0.0, pooled=0.0, ratio=0.0, lag1=0.0, neighbour=0.0)
    for b in BOUNCES:
        for r in range(reps):
            idx, sa = m.path_samples(pid, plain, LIGHT, b, N_FRAMES, np.random.default_rng([b, r, 1]))
            _, sm = m.path_samples(pid, plain, LIGHT, b, M_SAMPLES, np.random.default_rng([b, r, 2]))
            mean_a, _ = rr.moments(sa)
            mean_m, var_m = rr.moments(sm)
            z, zp, pooled, pse = channel_stats(mean_a, N_FRAMES, mean_m, var_m, M_SAMPLES)
            x = sa.astype(np.float64).mean(2)
            st = independence_stats(x)
            nb, znb, npairs = neighbour_stat(x, idx, w)
            print(f"bounces {b} rep {r}: worst |z| {np.abs(z).max():.2f} z sd {z[var_m > 0].std():.3f} pooled {pooled:+.4f} "
                  f"+- {pse:.4f} (z {zp:+.2f}) ratio {st['ratio'][0]:.3f} (z {st['ratio'][1]:+.2f}) lag1 {st['lag1'][0]:+.4f} "
                  f"(z {st['lag1'][1]:+.2f}) neighbour {nb:+.5f} / {npairs} pairs (z {znb:+.2f})", flush=True)
            for k, val in (("channel", np.abs(z).max()), ("pooled", abs(zp)), ("ratio", abs(st["ratio"][1])),
                           ("lag1", abs(st["lag1"][1])), ("neighbour", abs(znb))):
                worst[k] = max(worst[k], float(val))
    print("worst:", {k: round(val, 3) for k, val in worst.items()})
    return worst


if __name__ == "__main__" and sys.argv[1:2] == ["calibrate"]:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import py_oracle as po
    osc = po.OracleScene(po.cgltrace.load(scene_file("interreflection")))
    plain_, pid_, _, _ = po.rt_render(osc, po.rt_params(32, 32, shadows=False))   # raster-pinned inputs only
    calibrate(pid_, plain_)
