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
