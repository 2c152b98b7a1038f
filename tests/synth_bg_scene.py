"""A small synthetic .cgltrace scene for the background-layer table
(rt_common.h rt_bglayer_t): drawcall 0, depth test off, holds three screen
layers -- a pair of triangles that covers the whole screen (split along the
diagonal, like tekkaman's backdrop quad) and a third, small triangle in one
corner, drawn last, so blocks are crossed by its edges and by the diagonal;
drawcall 1 is a few small depth-tested triangles at the centre, so a frame has
heavy tiles and a background tier behind them."""
import re

import numpy as np

from conftest import scene_path
from synth_scene import LAYER_HEAD_STATES, _drawcall_xml

LAYER_PIDS = (0, 1, 2)


def _tris(corners, w=100.0, depth=0.5):
    """corners: [n][3] (x, y) in NDC -> verts as synth_scene._geometry_xml takes them"""
    c = np.asarray(corners, np.float64)
    n = c.shape[0]
    ww = np.full(n, w)
    return [(c[:, k, 0] * ww, c[:, k, 1] * ww, ww * depth, ww) for k in range(3)]


def make_bg_scene(path: str) -> str:
    tmpl = open(scene_path("triangle")).read()
    start = tmpl.index('<item class_id="2"')
    end = tmpl.index("</drawcalls>")
    item = tmpl[start:end]
    e = 1.25  # past the screen's edges: every pixel centre is covered
    layers = _tris([[(-e, -e), (e, -e), (e, e)], [(-e, -e), (e, e), (-e, e)],
                    [(-0.97, -0.93), (-0.41, -0.88), (-0.83, -0.37)]])
    rng = np.random.default_rng(11)
    ctr = rng.uniform(-0.12, 0.12, (4, 1, 2)) + rng.uniform(-0.06, 0.06, (4, 3, 2))
    geom = _tris(ctr, depth=0.4)
    calls = [_drawcall_xml(item, {}, layers, np.array([[0.9, 0.2, 0.2], [0.2, 0.9, 0.2], [0.2, 0.2, 0.9]]), 1.0),
             re.sub(r' class_id="\d+" tracking_level="\d+" version="\d+"', "",
                    _drawcall_xml(item, LAYER_HEAD_STATES, geom, np.full((4, 3), 0.7), 1.0))]
    xml = tmpl[:start].replace("<count>1</count>", f"<count>{len(calls)}</count>") + "".join(calls) + tmpl[end:]
    with open(path, "w") as f:
        f.write(xml)
    return path
