"""Synthetic .cgltrace scenes for tests that need more triangles than the
reference's scenes hold (the GPU BVH builder's multi-block radix sort).
Same XML layout as the reference's traces (tests/golden/scenes/triangle.
cgltrace: boost_serialization v15); one depth-tested (LESS) drawcall of n
random triangles in clip space, w in [90, 110] like tekkaman's model."""
import gzip
import os
import re

import numpy as np

from conftest import scene_path

_ITEM0 = ('<item class_id="6" tracking_level="0" version="0"><first>{i}</first>'
          '<second class_id="7" tracking_level="0" version="0">'
          '<pos class_id="8" tracking_level="0" version="0"><x>{x:.9e}</x><y>{y:.9e}</y>'
          '<z>{z:.9e}</z><w>{w:.9e}</w></pos><color><r>{r:.9e}</r><g>{g:.9e}</g><b>{b:.9e}</b>'
          '<a>{a:.9e}</a></color><texcoord class_id="9" tracking_level="0" version="0">'
          '<u>0.000000000e+00</u><v>0.000000000e+00</v></texcoord></second></item>')
_ITEM = ('<item><first>{i}</first><second><pos><x>{x:.9e}</x><y>{y:.9e}</y><z>{z:.9e}</z>'
         '<w>{w:.9e}</w></pos><color><r>{r:.9e}</r><g>{g:.9e}</g><b>{b:.9e}</b>'
         '<a>{a:.9e}</a></color><texcoord><u>0.000000000e+00</u><v>0.000000000e+00</v>'
         '</texcoord></second></item>')


def make_scene(path: str, n: int, seed: int = 1, size: float = 0.03, w_range=(90.0, 110.0),
               spread: float = 0.8, w_jitter: float = 0.5, degenerate: int = 0) -> str:
    """Writes a gzip'd trace of n triangles to `path` (returned): centres
    uniform in +-spread (NDC), corners +-size around them, w in w_range,
    each corner's w jittered by +-w_jitter (w_jitter > w_range[0] puts some
    corners behind the eye); the first `degenerate` triangles repeat their
    first corner as their last (zero area: the setup's det == 0 exactly)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(w_range[0], w_range[1], n)
    cx, cy = rng.uniform(-spread, spread, n) * w, rng.uniform(-spread, spread, n) * w
    verts = []
    for k in range(3):
        ox, oy = rng.uniform(-size, size, n) * w, rng.uniform(-size, size, n) * w
        dw = rng.uniform(-w_jitter, w_jitter, n)
        verts.append((cx + ox, cy + oy, (w + dw) * 0.5, w + dw))
    if degenerate:
        verts[2] = tuple(np.concatenate([v0[:degenerate], v2[degenerate:]])
                         for v0, v2 in zip(verts[0], verts[2]))
    col = rng.uniform(0.2, 1.0, (n, 3))
    return _write(path, verts, col)


def make_chain_scene(path: str, n: int, ratio: float = 1.6, base: float = 1e-3) -> str:
    """n small triangles whose x centres grow geometrically (base * ratio^k,
    NDC): every binned-SAH split peels a few off the far end, so the tree is
    about n / 5 levels deep -- deeper than the device build's level budget
    (log2 n + 4) for n = 96."""
    k = np.arange(n, dtype=np.float64)
    w = np.full(n, 100.0)
    cx = base * ratio ** k * w
    verts = [(cx + dx * w, np.full(n, dy) * w, w * 0.5, w) for dx, dy in ((0.0, 0.0), (0.01, 0.0), (0.0, 0.01))]
    return _write(path, verts, np.full((n, 3), 0.5))


# ---- scenes for the RT model (tests/rt_reference.py) ------------------------
# One flat colour per triangle, no texture: the plain frame shows a triangle
# in floor(c * 255) per channel, which the model takes as its albedo.

def make_interreflection_scene(path: str) -> str:
    """48 large overlapping triangles (corners up to 8 apart in w), so that
    bounce rays hit often: ~330 path pixels at 32x32, mean radiance ~45/255"""
    return make_scene(path, n=48, seed=5, size=0.35, spread=0.6, w_jitter=8.0)


def _tris_to_verts(tris):
    """[(corner, corner, corner)] of clip (x, y, w) -> _write's verts; depth
    z / w = 1 - 50 / w grows with w, so the raster's winner is the nearest"""
    t = np.asarray(tris, np.float64)
    return [(t[:, k, 0], t[:, k, 1], t[:, k, 2] - 50.0, t[:, k, 2]) for k in range(3)]


def _quad(a, b, c, d):
    return [(a, b, c), (a, c, d)]


def make_convex_scene(path: str) -> str:
    """One tilted quad (two triangles sharing the diagonal) facing the default
    light and nothing else: no bounce ray can hit, no shadow segment is
    blocked, so a path frame is alb0 * (cos + 0.25) whatever the seed."""
    w = lambda x, y: 100.0 + 0.08 * x + 0.05 * y
    p = [(x, y, w(x, y)) for x, y in ((-60.0, -50.0), (60.0, -50.0), (60.0, 50.0), (-60.0, 50.0))]
    tris = _quad(*p)
    return _write(path, _tris_to_verts(tris), np.tile([[0.8, 0.6, 0.4]], (2, 1)))


SHADOW_EDGE_LIGHTS = [(10.0, 30.0, 85.0),        # close to the geometry
                      (0.0, 60.0, 80.0),         # the default light
                      (-150.0, 400.0, -200.0)]   # far away, behind the eye


def make_shadow_edge_scene(path: str) -> str:
    """A tilted wall behind occluders whose silhouettes cross many pixels: a
    sliver, a quad of two triangles sharing an edge (a ray through the seam must
    hit), a comb of narrow spikes; a large triangle beyond the close light (on
    the line wall -> light past the light: it must not shadow, off screen); a
    large triangle behind the wall (met by the segment's line before its
    start); a quad whose eye side faces away from the two near lights (its own
    plane lies between its pixels' origins and the light)."""
    ww = lambda x, y: 110.0 + 0.05 * x - 0.03 * y
    wall = [(x, y, ww(x, y)) for x, y in ((-100.0, -100.0), (100.0, -100.0), (100.0, 100.0), (-100.0, 100.0))]
    tris = _quad(*wall)
    tris.append(((-60.0, -40.0, 100.0), (60.0, 30.0, 98.0), (58.0, 36.0, 99.0)))          # sliver
    ws = lambda x: 97.0 + 0.1 * x
    tris += _quad((-30.0, 10.0, ws(-30.0)), (0.0, 10.0, ws(0.0)), (0.0, 40.0, ws(0.0)), (-30.0, 40.0, ws(-30.0)))
    for k in range(6):                                                                     # comb
        tris.append(((20.0 + 8 * k, -60.0, 101.0), (19.0 + 8 * k, -10.0, 99.0), (16.0 + 8 * k, -10.0, 99.0)))
    tris.append(((-200.0, 70.0, 60.0), (250.0, 70.0, 60.0), (0.0, 400.0, 58.0)))          # beyond the light
    tris.append(((-150.0, -150.0, 130.0), (150.0, -150.0, 130.0), (0.0, 200.0, 130.0)))   # behind the wall
    tris += _quad((-50.0, -45.0, 88.0), (50.0, -45.0, 88.0), (50.0, -75.0, 106.0), (-50.0, -75.0, 106.0))
    col = np.random.default_rng(11).uniform(0.3, 1.0, (len(tris), 3))
    return _write(path, _tris_to_verts(tris), col)


def _geometry_xml(verts, col, alpha: float = 1.0) -> str:
    """the <vertices> and <primitives> elements of one drawcall"""
    n = len(col)
    items = []
    for t in range(n):
        for k in range(3):
            x, y, z, ww = (float(a[t]) for a in verts[k])
            fmt = _ITEM0 if not items else _ITEM
            items.append(fmt.format(i=3 * t + k, x=x, y=y, z=z, w=ww, r=col[t, 0], g=col[t, 1],
                                    b=col[t, 2], a=alpha))
    prims = ['<item class_id="11" tracking_level="0" version="0"><i0>0</i0><i1>1</i1><i2>2</i2></item>']
    prims += [f"<item><i0>{3 * t}</i0><i1>{3 * t + 1}</i1><i2>{3 * t + 2}</i2></item>"
              for t in range(1, n)]
    return (f'<vertices class_id="5" tracking_level="0" version="0"><count>{3 * n}</count>'
            f'<bucket_count>{3 * n}</bucket_count><item_version>0</item_version>' + "".join(items) +
            '</vertices><primitives class_id="10" tracking_level="0" version="0">'
            f'<count>{n}</count><item_version>0</item_version>' + "".join(prims) + "</primitives>")


def _write(path, verts, col):
    tmpl = open(scene_path("triangle")).read()
    head, rest = tmpl.split('<vertices class_id="5"', 1)
    head = head.replace("<depth_test>0</depth_test>", "<depth_test>1</depth_test>")
    head = head.replace("<depth_func>0</depth_func>", "<depth_func>1</depth_func>")
    head = head.replace("<depth_writemask>0</depth_writemask>", "<depth_writemask>1</depth_writemask>")
    tail = rest.split("</primitives>", 1)[1]
    xml = head + _geometry_xml(verts, col) + tail
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with gzip.open(path, "wt") as f:
        f.write(xml)
    return path


# ---- a small layered scene for the output-merger state sweeps ---------------
# An opaque LESS head, then tail drawcalls whose states the caller chooses.
# Tail drawcalls re-submit some of the head's (and each other's) triangles
# vertex for vertex -- exact depth ties -- next to new triangles in front of
# and behind what is there, so all three outcomes of a depth compare occur,
# and overdraw runs from 0 to more than 3 layers across the frame.
LAYER_HEAD_STATES = dict(depth_test=1, depth_func=1, depth_writemask=1)


def _layer_tris(rng, n, size, depth_range):
    """n triangles: (verts as in _write, colours [n, 3]); a corner's depth
    z / w is uniform in depth_range, w is the triangle's (90..110)"""
    w = rng.uniform(90.0, 110.0, n)
    cx, cy = rng.uniform(-0.75, 0.75, n), rng.uniform(-0.75, 0.75, n)
    verts = []
    for _ in range(3):
        ox, oy = rng.uniform(-size, size, n), rng.uniform(-size, size, n)
        zn = rng.uniform(depth_range[0], depth_range[1], n)
        verts.append(((cx + ox) * w, (cy + oy) * w, zn * w, w))
    return verts, rng.uniform(0.15, 1.0, (n, 3))


def _pick(tris, idx):
    verts, col = tris
    return [tuple(a[idx] for a in v) for v in verts], col[idx]


def _join(*parts):
    verts = [tuple(np.concatenate([p[0][k][c] for p in parts]) for c in range(4)) for k in range(3)]
    return verts, np.concatenate([p[1] for p in parts])


def layer_geometry(seed: int = 3):
    """[head, tail 1, tail 2, tail 3] triangle sets of the layered scene;
    tail 3 is tail 2 again, so a third drawcall can read back what the second
    left in the depth/stencil plane"""
    rng = np.random.default_rng(seed)
    head = _layer_tris(rng, 20, 0.4, (0.35, 0.65))
    near1, far1 = _layer_tris(rng, 6, 0.35, (0.1, 0.3)), _layer_tris(rng, 6, 0.35, (0.7, 0.9))
    tail1 = _join(_pick(head, np.arange(0, 8)), near1, far1)
    near2, far2 = _layer_tris(rng, 5, 0.35, (0.05, 0.45)), _layer_tris(rng, 5, 0.35, (0.55, 0.95))
    tail2 = _join(_pick(head, np.arange(4, 14)), _pick(near1, np.arange(0, 3)),
                  _pick(far1, np.arange(0, 3)), near2, far2)
    return [head, tail1, tail2, tail2]


def _drawcall_xml(template_item: str, states: dict, verts, col, alpha: float) -> str:
    xml = template_item
    for tag, value in states.items():
        assert xml.count(f"<{tag}>") == 1, tag
        head, rest = xml.split(f"<{tag}>", 1)
        xml = head + f"<{tag}>{int(value)}" + rest[rest.index(f"</{tag}>"):]
    head, rest = xml.split('<vertices class_id="5"', 1)
    return head + _geometry_xml(verts, col, alpha) + rest.split("</primitives>", 1)[1]


def make_layer_scene(path: str, tail_states, seed: int = 3, tail_alpha=(0.625, 0.375, 0.5)) -> str:
    """Writes the layered scene (plain text) to `path` (returned): drawcall 0
    is the opaque head (LAYER_HEAD_STATES), drawcall 1 + i carries
    tail_states[i] (trace state tags -> values, on top of the template's
    all-off states) and vertex alpha tail_alpha[i].  Three tail drawcalls."""
    assert len(tail_states) == 3
    tmpl = open(scene_path("triangle")).read()
    start = tmpl.index('<item class_id="2"')
    end = tmpl.index("</drawcalls>")
    item = tmpl[start:end]
    geo = layer_geometry(seed)
    calls = [_drawcall_xml(item, LAYER_HEAD_STATES, *geo[0], 1.0)]
    for st, g, a in zip(tail_states, geo[1:], tail_alpha):
        # boost writes a class's attributes at its first occurrence only
        calls.append(re.sub(r' class_id="\d+" tracking_level="\d+" version="\d+"', "",
                            _drawcall_xml(item, st, *g, a)))
    xml = (tmpl[:start].replace("<count>1</count>", f"<count>{len(calls)}</count>") + "".join(calls) +
           tmpl[end:])
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(xml)
    return path
