"""The shading keys rt_kernel is specialised on (gfx_device.h GFX_SHADE_KEYS:
shade_wave branches once per wave-uniform drawcall to a shade() instantiated
on the drawcall's COLOR / TEX / MODULATE flags, filter, wraps and format)
must be the textured keys the golden scenes use most.  CPU test: the keys are
restated from the traces with the rules of app/setup.cpp DrawcallState and
the specialised set is read from the header."""
import collections
import glob
import os
import re

from conftest import GOLDEN, ROOT

from oracle import cgltrace

RT_DC_COLOR, RT_DC_TEX, RT_DC_MODULATE = 0x2, 0x4, 0x8
FILTER_POINT, FILTER_BILINEAR = 0, 1
WRAP_CLAMP, WRAP_REPEAT = 0, 1
# VX_types.h formats by the trace's format code (setup.cpp ToVXFormat) and their strides
VX_FORMAT = {1: ("VX_TEX_FORMAT_A8", 1), 2: ("VX_TEX_FORMAT_L8", 1), 3: ("VX_TEX_FORMAT_A8L8", 2),
             4: ("VX_TEX_FORMAT_R5G6B5", 2)}
HEADER = os.path.join(ROOT, "skybox_rt_amd", "csrc", "kernels", "gfx_device.h")


def scene_names():
    return sorted(os.path.basename(p).split(".")[0] for p in glob.glob(os.path.join(GOLDEN, "scenes", "*")))


def load(name):
    for ext in (".cgltrace", ".cgltrace.gz"):
        p = os.path.join(GOLDEN, "scenes", name + ext)
        if os.path.exists(p):
            return cgltrace.load(p)
    raise FileNotFoundError(name)


def rt_accepts(scene):
    """rt_app.cpp: the RT path rejects blending, stencil and partial colour masks"""
    return all(not dc.states["blend_enabled"] and not dc.states["stencil_test"] and
               (dc.states["color_writemask"] & 0xf) == 0xf for dc in scene.drawcalls)


def drawcall_key(scene, dc):
    """(flags, filter, wrapu, wrapv, format name, stride) as DrawcallState derives them"""
    s = dc.states
    color, tex = s["color_enabled"] != 0, s["texture_enabled"] != 0
    modulate = tex and s["texture_envmode"] == 3 and color
    if tex and color and not modulate:
        color = False
    t = scene.textures.get(dc.texture_id)
    if tex and t is None:
        tex = False
    flags = (RT_DC_COLOR if color else 0) | (RT_DC_TEX if tex else 0) | (RT_DC_MODULATE if modulate else 0)
    if not tex:
        return (flags, 0, 0, 0, "VX_TEX_FORMAT_A8R8G8B8", 0)
    fmt, stride = VX_FORMAT.get(t[0], ("VX_TEX_FORMAT_A8R8G8B8", 4))
    filt = FILTER_BILINEAR if s["texture_magfilter"] != 1 else FILTER_POINT
    wrap = WRAP_REPEAT if s["texture_addressU"] == 0 else WRAP_CLAMP
    return (flags, filt, wrap, wrap, fmt, stride)


def specialised_keys():
    """the X(flags, format, stride) rows of GFX_SHADE_KEYS (bilinear, REPEAT / REPEAT)"""
    src = open(HEADER).read()
    body = src[src.index("#define GFX_SHADE_KEYS(X)"):]
    body = body[:body.index("\n//")]
    flag_bits = {"RT_DC_COLOR": RT_DC_COLOR, "RT_DC_TEX": RT_DC_TEX, "RT_DC_MODULATE": RT_DC_MODULATE}
    keys = set()
    rows = re.findall(r"X\(([^,]+),\s*(VX_TEX_FORMAT_\w+),\s*(\d+)u?\)", body)
    # every X(...) row of the macro is understood (the macro's own `(X)` parameter aside)
    assert len(rows) == body.count("X(") > 0, body
    for flags, fmt, stride in rows:
        bits = 0
        for f in flags.split("|"):
            bits |= flag_bits[f.strip()]
        keys.add((bits, FILTER_BILINEAR, WRAP_REPEAT, WRAP_REPEAT, fmt, int(stride)))
    return keys


def test_specialised_keys_cover_the_most_used_textured_keys():
    use = collections.Counter()  # primitives per textured key, RT-accepted golden scenes
    for name in scene_names():
        sc = load(name)
        if not rt_accepts(sc):
            continue
        for dc in sc.drawcalls:
            k = drawcall_key(sc, dc)
            if k[0] & RT_DC_TEX:
                use[k] += dc.prim_count
    assert use, "no textured drawcall in the golden scenes"
    spec = specialised_keys()
    assert 1 <= len(spec) <= 4
    print("textured keys by primitives:", use.most_common(), "specialised:", sorted(spec))
    # every specialised key is in use, and no unspecialised key is used more
    # than a specialised one
    assert spec <= set(use), f"specialised keys no golden scene uses: {spec - set(use)}"
    least = min(use[k] for k in spec)
    others = [n for k, n in use.items() if k not in spec]
    assert not others or max(others) < least, (use, spec)
    # the benchmark scene's drawcalls are all specialised
    tek = load("tekkaman")
    assert {drawcall_key(tek, dc) for dc in tek.drawcalls} <= spec


def test_accepted_scenes_are_the_unblended_ones():
    acc = {n for n in scene_names() if rt_accepts(load(n))}
    assert acc == {"box", "carnival", "scene", "tekkaman", "triangle"}
