"""Synthetic textured .cgltrace scenes: the golden `box` trace (two textured
drawcalls, bilinear, REPEAT / REPEAT, one 128x128 R5G6B5 texture) with its
sampler state or its texture's format rewritten, so that a drawcall differs
from the shading keys rt_kernel is specialised on (gfx_device.h
GFX_SHADE_KEYS) in exactly the wraps, or the format, or format and stride:

  clamp     texture_addressU 1: CLAMP / CLAMP (wrapV follows addressU), R5G6B5
  a8l8      REPEAT, the same texel bytes read as A8L8 (stride 2)
  argb8888  REPEAT, the same texel bytes read as a 128x64 A8R8G8B8 texture
            (stride 4)
"""
import gzip
import os
import re

from conftest import scene_path

VARIANTS = ("clamp", "a8l8", "argb8888")


def make_tex_scene(path: str, variant: str) -> str:
    xml = open(scene_path("box")).read()
    if variant == "clamp":
        xml, n = re.subn(r"<texture_addressU>0</texture_addressU>", "<texture_addressU>1</texture_addressU>", xml)
        assert n == 2
    elif variant == "a8l8":
        xml, n = re.subn(r"<format>4</format>", "<format>3</format>", xml)
        assert n == 1
    elif variant == "argb8888":
        xml, n = re.subn(r"<format>4</format>(\s*)<width>128</width>(\s*)<height>128</height>",
                         r"<format>5</format>\1<width>128</width>\2<height>64</height>", xml)
        assert n == 1
    else:
        raise ValueError(variant)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with gzip.open(path, "wt") as f:
        f.write(xml)
    return path
