"""Shared helpers of the ordered-tail tests (test_om_layers_cpu.py,
test_gpu_om_layers.py): the scenes whose drawcalls the RT path cannot trace as
a whole, the split rule restated, the composed checker, and vase with one
tail drawcall's states rewritten.

The composed checker defines the frame of a scene loaded with om_layers=True
(include/vx_rt.h RT_SCENE_OM_LAYERS) from the oracle's two pinned renderers:
the head (the drawcalls before the first one the RT path cannot trace) by the
oracle's ray tracer (with shadows) or its raster pipeline (without), the
head's depth/stencil buffer by the raster pipeline, and the tail by the raster
pipeline again, on top of those two buffers.

Run as a program it renders one frame on the GPU and saves it (the child
process of the tests that set the list switches in the environment):
    python tests/om_scenes.py <scene file> <size> <shadows 0|1> <out.npy>
"""
import ctypes as C
import functools
import gzip
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCENES = ("vase", "mouse", "evilskull", "polybump")
# (first tail drawcall, tail primitives) of the four golden scenes
SPLITS = {"vase": (2, 542), "mouse": (8, 34), "evilskull": (2, 44), "polybump": (1, 96)}
DEFAULT_LIGHT = (0.0, 60.0, 80.0)
DEPTH_LESS, DEPTH_LEQUAL = 1, 3   # cgltrace depth_func indices (gfxutil.cpp:296-311)


def scene_file(name):
    for ext in (".cgltrace", ".cgltrace.gz"):
        p = os.path.join(ROOT, "tests", "golden", "scenes", name + ext)
        if os.path.exists(p):
            return p
    raise FileNotFoundError(name)


def first_tail_drawcall(scene) -> int:
    """The first drawcall that breaks a rule of the RT path's classification
    (no blending, no stencil, full colour mask; depth-tested drawcalls write
    depth; one LESS or LEQUAL depth function throughout; screen layers only
    before geometry), or the drawcall count."""
    seen_geom, func = False, None
    for d, dc in enumerate(scene.drawcalls):
        s = dc.states
        if s["blend_enabled"] or s["stencil_test"] or (s["color_writemask"] & 0xF) != 0xF:
            return d
        if s["depth_test"]:
            f = s["depth_func"]
            if not (s["depth_writemask"] & 1) or f not in (DEPTH_LESS, DEPTH_LEQUAL) \
                    or (func is not None and f != func):
                return d
            func, seen_geom = f, True
        elif seen_geom:
            return d
    return len(scene.drawcalls)


@functools.lru_cache(maxsize=None)
def load_full(path):
    from oracle import py_oracle as po
    return po.cgltrace.load(path)


@functools.lru_cache(maxsize=None)
def composed(path, width, height, shadows, light=DEFAULT_LIGHT):
    """The expected frame of scene file `path` loaded with om_layers=True:
    (colour uint32[H, W], depth/stencil uint32[H, W], the head's ray counters
    or None without shadows).  Computed once per case; callers must not write
    into the arrays."""
    from oracle import py_oracle as po
    full = load_full(path)
    k = first_tail_drawcall(full)
    n = len(full.drawcalls)
    head = po.OracleScene(po.cgltrace.select_drawcalls(full, range(k)))
    tail = po.OracleScene(po.cgltrace.select_drawcalls(full, range(k, n)))
    rc, rd, _ = po.raster_render(head, width, height)
    counters = None
    if shadows:
        color, _, _, counters = po.rt_render(head, po.rt_params(width, height, shadows=True, light=light))
    else:
        color = rc
    color = np.ascontiguousarray(color, np.uint32).reshape(-1).copy()
    depth = np.ascontiguousarray(rd, np.uint32).reshape(-1).copy()
    pid = np.empty(width * height, np.int32)
    rv = po.lib().orc_raster_render(C.byref(tail.c), width, height, 5, color.ctypes.data,
                                    depth.ctypes.data, pid.ctypes.data)
    assert rv == 0, rv
    color, depth = color.reshape(height, width), depth.reshape(height, width)
    color.setflags(write=False)
    depth.setflags(write=False)
    return color, depth, counters


@functools.lru_cache(maxsize=None)
def raster_full(path, width, height):
    """The oracle's raster frame of the whole scene: (colour, depth/stencil)."""
    from oracle import py_oracle as po
    c, d, _ = po.raster_render(po.OracleScene(load_full(path)), width, height)
    c.setflags(write=False)
    d.setflags(write=False)
    return c, d


# ---- vase with one tail drawcall's states rewritten --------------------------
# state values are the trace's indices (gfxutil.cpp:296-346): compare 2 = EQUAL;
# stencil op 4 = ZERO; blend 8 = DST_RGB, 3 = ONE_MINUS_SRC_RGB
MUTATIONS = {
    # drawcall 3 (blended, depth-tested) writes only green and alpha
    "mask": [(3, "color_writemask", 0xA)],
    # drawcall 4 (a blended depth-off overlay): stencil EQUAL 0xff against the
    # cleared 0xff plane, zeroed where a fragment passes -- the first fragment
    # of a pixel passes, every later one of the drawcall there fails (its
    # primitives overlap in places).  (The trace's stencil_zfail drives the
    # pass operation: draw3d writes ZPASS twice, main.cpp:251-260.)
    "stencil": [(4, "stencil_test", 1), (4, "stencil_func", 2), (4, "stencil_ref", 0xFF),
                (4, "stencil_mask", 0xFF), (4, "stencil_writemask", 0xFF), (4, "stencil_zpass", 4),
                (4, "stencil_zfail", 4), (4, "stencil_fail", 0)],
    # drawcall 2 (blended, depth-tested) blends DST_RGB / ONE_MINUS_SRC_RGB
    "blend": [(2, "blend_src", 8), (2, "blend_dst", 3)],
}
MUTATIONS["all"] = MUTATIONS["mask"] + MUTATIONS["stencil"] + MUTATIONS["blend"]


def rewrite_states(text: str, edits) -> str:
    """`edits`: (drawcall n, state tag, value); replaces the n-th
    <tag>...</tag> of the trace's text (every drawcall carries each state tag
    once, and nothing else is named like a state)."""
    for n, tag, value in edits:
        hits = list(re.finditer(rf"<{tag}>[^<]*</{tag}>", text))
        assert len(hits) > n, (tag, len(hits))
        m = hits[n]
        text = text[:m.start()] + f"<{tag}>{value}</{tag}>" + text[m.end():]
    return text


def mutated_vase(directory, which: str) -> str:
    """Write vase with MUTATIONS[which] applied into `directory`; the path."""
    out = os.path.join(str(directory), f"vase_{which}.cgltrace")
    if not os.path.exists(out):
        with gzip.open(scene_file("vase"), "rt") as f:
            text = f.read()
        with open(out, "w") as f:
            f.write(rewrite_states(text, MUTATIONS[which]))
    return out


# ---- the layered synthetic scene, one tail state swept at a time ---------------
# (tests/synth_scene.py make_layer_scene: an opaque LESS head and three tail
# drawcalls with exact depth ties, nearer and farther fragments and 0 to 3+
# layers of overdraw.)  State values are the trace's indices: compare 0 NEVER,
# 1 LESS, 2 EQUAL, 3 LEQUAL, 4 GREATER, 5 NOTEQUAL, 6 GEQUAL, 7 ALWAYS; stencil
# op 0 KEEP, 1 REPLACE, 2 INCR, 3 DECR, 4 ZERO, 5 INVERT; blend 0 ZERO, 1 ONE,
# 2 SRC_RGB, 3 1-SRC_RGB, 4 SRC_A, 5 1-SRC_A, 6 DST_A, 7 1-DST_A, 8 DST_RGB,
# 9 1-DST_RGB, 10 ALPHA_SAT.  The pass operation is the trace's stencil_zfail
# (the draw3d quirk above).
#
# Tail drawcall 1 counts: LEQUAL without depth writes, stencil ALWAYS / DECR from
# the cleared 0xff, alpha-blended -- it leaves stencil values 0xff, 0xfe, 0xfd,
# ... and destination alphas other than 0xff for tail drawcall 2, the swept one.
# Tail drawcall 3 reads back: drawcall 2's triangles again, depth test off,
# blended where the stencil's low two bits are EQUAL 0xfe's (so 0xfe and INVERT's
# 0x02 pass, 0xff, 0xfd, 0xfc, 0x00 and 0x01 fail), writing no stencil -- what
# drawcall 2 left in the stencil plane shows in the colour plane, the only
# plane the om_layers path exposes.
LAYER_COUNTING = dict(depth_test=1, depth_func=3, depth_writemask=0, stencil_test=1, stencil_func=7,
                      stencil_zpass=3, stencil_zfail=3, stencil_fail=0, stencil_ref=0,
                      stencil_mask=0xFF, stencil_writemask=0xFF, blend_enabled=1, blend_src=4,
                      blend_dst=5)
LAYER_READER = dict(stencil_test=1, stencil_func=2, stencil_ref=0xFE, stencil_mask=0x03,
                    stencil_writemask=0, blend_enabled=1, blend_src=4, blend_dst=5)
LAYER_SWEPT = dict(depth_test=1, depth_func=3, depth_writemask=1, blend_enabled=1, blend_src=4,
                   blend_dst=5, color_writemask=0xF)
_STENCIL = dict(stencil_test=1, stencil_ref=0xFE, stencil_mask=0xFF, stencil_writemask=0xFF)
# family -> (values, the swept drawcall's states for value v)
LAYER_FAMILIES = {
    "depth_func": (range(8), lambda v: dict(depth_func=v)),
    "stencil_func": (range(8), lambda v: dict(_STENCIL, stencil_func=v, stencil_zpass=5,
                                              stencil_zfail=5, stencil_fail=4)),
    "pass_op": (range(6), lambda v: dict(_STENCIL, stencil_func=7, stencil_zpass=v, stencil_zfail=v,
                                         stencil_fail=0)),
    "fail_op": (range(6), lambda v: dict(_STENCIL, stencil_func=2, stencil_zpass=2, stencil_zfail=2,
                                         stencil_fail=v)),
    "blend_src": (range(11), lambda v: dict(blend_src=v)),
    "blend_dst": (range(11), lambda v: dict(blend_dst=v)),
    "color_writemask": (range(16), lambda v: dict(color_writemask=v)),
}
LAYER_CASES = [(f, v) for f, (values, _) in LAYER_FAMILIES.items() for v in values]


def layer_scene(directory, family: str, value: int) -> str:
    """Write the layered scene with `family` = value on its swept drawcall
    into `directory`; the path."""
    from synth_scene import make_layer_scene
    out = os.path.join(str(directory), f"layers_{family}_{value}.cgltrace")
    if not os.path.exists(out):
        make_layer_scene(out, [LAYER_COUNTING, dict(LAYER_SWEPT, **LAYER_FAMILIES[family][1](value)),
                               LAYER_READER])
    return out


# vase's own sweeps (a real scene): (family, drawcall, values)
VASE_SWEEPS = (("blend_src", 4, range(11)), ("blend_dst", 4, range(11)), ("color_writemask", 3, range(16)))
VASE_CASES = [(tag, dc, v) for tag, dc, values in VASE_SWEEPS for v in values]


def swept_vase(directory, tag: str, drawcall: int, value: int) -> str:
    out = os.path.join(str(directory), f"vase_{tag}_{drawcall}_{value}.cgltrace")
    if not os.path.exists(out):
        with gzip.open(scene_file("vase"), "rt") as f:
            text = f.read()
        with open(out, "w") as f:
            f.write(rewrite_states(text, [(drawcall, tag, value)]))
    return out


# ---- GPU side ------------------------------------------------------------------
def gpu_frame(path, width, height, shadows, counters=False, **kw):
    """One frame of `path` loaded with om_layers=True -> (framebuffer, stats)."""
    from skybox_rt_amd import rt
    s = rt.Scene.load(path, om_layers=True)
    r = rt.Renderer(s)
    try:
        r.configure(width, height, shadows=shadows, counters=counters, **kw)
        r.render()
        return r.framebuffer(), (r.stats() if counters else None)
    finally:
        r.close()
        s.close()


if __name__ == "__main__":
    fb, _ = gpu_frame(sys.argv[1], int(sys.argv[2]), int(sys.argv[2]), bool(int(sys.argv[3])))
    np.save(sys.argv[4], fb)
