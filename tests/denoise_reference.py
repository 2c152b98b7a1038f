"""The denoiser's definition (vx_rt.h, "Denoising accumulated path frames") in
numpy, written from that text and not from the kernels: plain per-tap loops
over shifted arrays, uint64 where a product passes 32 bits.  The device frame
must equal denoise() on the read-back inputs bit for bit
(tests/test_gpu_denoise.py); tests/test_denoise_model_cpu.py pins this model
itself to hand-worked answers.

Inputs, all [H, W] unless noted:
  rec     uint32 [H, W, 4]  accumulation records {s_R, s_G, s_B, n}, n >= 1
  pid     int32             guide primitive
  z       uint32            24-bit depth word
  geom    bool              RT_AOV_GEOM
  base    uint32            ARGB base colour A
  normal  int [H, W, 3]     guide normal N, each component a signed byte
"""
import numpy as np

B = (1, 4, 6, 4, 1)
RT_AOV_GEOM = 0x01000000


def channels(argb):
    """R, G, B of ARGB words as uint64 [..., 3]"""
    a = np.asarray(argb).astype(np.uint64)
    return np.stack([(a >> np.uint64(16)) & np.uint64(0xFF), (a >> np.uint64(8)) & np.uint64(0xFF),
                     a & np.uint64(0xFF)], -1)


def pack(alpha_argb, rgb):
    """alpha(alpha_argb) | R << 16 | G << 8 | B"""
    rgb = np.asarray(rgb).astype(np.uint64)
    v = (rgb[..., 0] << np.uint64(16)) | (rgb[..., 1] << np.uint64(8)) | rgb[..., 2]
    return (np.asarray(alpha_argb).astype(np.uint64) & np.uint64(0xFF000000) | v).astype(np.uint32)


def accum_resolve(rec, alpha_argb):
    """rt_accum_resolve: alpha over the rounded means (2 s + n) // (2 n), clamped to 255; n = 0: alpha alone"""
    rec = np.asarray(rec).astype(np.uint64)
    n = rec[..., 3:4]
    m = np.where(n > 0, (2 * rec[..., :3] + n) // np.maximum(2 * n, 1), 0)
    return pack(alpha_argb, np.minimum(m, 255))


def stop(e):
    """E(e) = e >= 9 ? 0 : 256 >> e"""
    e = np.asarray(e).astype(np.int64)
    return np.where(e >= 9, 0, 256 >> np.minimum(e, 9)).astype(np.int64)


def demodulate(rec, base):
    """I_c = min(65535, (256 s_c + d // 2) // d), d = n * max(A_c, 1): int64 [H, W, 3]"""
    rec = np.asarray(rec).astype(np.uint64)
    d = rec[..., 3:4] * np.maximum(channels(base), 1)
    return np.minimum((np.uint64(256) * rec[..., :3] + d // np.uint64(2)) // d, 65535).astype(np.int64)


def shifted(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx] where that lies inside the image, else fill"""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if abs(dy) < H and abs(dx) < W:
        out[yd, xd] = a[ys, xs]
    return out


def one_pass(I, pid, z, geom, normal, k, zs, ls):
    """pass k (stride 2^(k-1)) over irradiance I int64 [H, W, 3]; pixels without geom keep their value"""
    st = 1 << (k - 1)
    H, W = pid.shape
    pid = pid.astype(np.int64)
    z = z.astype(np.int64)
    N = normal.astype(np.int64)
    num = np.zeros((H, W, 3), np.uint64)
    den = np.zeros((H, W), np.uint64)
    inside = np.ones((H, W), bool)
    for j in range(-2, 3):
        for i in range(-2, 3):
            h = B[i + 2] * B[j + 2]
            dx, dy = st * i, st * j
            ok = shifted(inside, dx, dy, False) & shifted(geom, dx, dy, False)
            Iq = shifted(I, dx, dy, 0)
            if i == 0 and j == 0:
                w = np.full((H, W), 256, np.int64)
            else:
                same = shifted(pid, dx, dy, -2) == pid
                wz = stop(np.abs(z - shifted(z, dx, dy, 0)) >> (zs + k - 1))
                c = np.minimum(256, np.abs((N * shifted(N, dx, dy, 0)).sum(-1)) >> 6)
                wn = (c * c) >> 8
                wn = (wn * wn) >> 8
                wz = np.where(same, 256, wz)
                wn = np.where(same, 256, wn)
                wl = stop(np.abs(I - Iq).max(-1) >> ls)
                w = (wz * wn * wl) >> 16
            hw = np.where(ok, h * w, 0).astype(np.uint64)
            den += hw
            num += hw[..., None] * Iq.astype(np.uint64)
    den1 = np.maximum(den, 1)
    total = num + (den1 // np.uint64(2))[..., None]
    assert int(total.max()) < 2 ** 32, "a sum left 32 bits"
    out = (total // den1[..., None]).astype(np.int64)
    return np.where(geom[..., None], out, I)


def store(I, rec, geom, base):
    """the stored frame of irradiance I: remodulated where geom, the accumulation resolve elsewhere"""
    rgb = np.minimum(255, (I.astype(np.uint64) * channels(base) + np.uint64(128)) >> np.uint64(8))
    return np.where(geom, pack(base, rgb), accum_resolve(rec, base))


def frames(rec, pid, z, geom, base, normal, passes, zs, ls):
    """the stored frames of passes = 1, 2, .. `passes`: pass k's input does not depend on how many follow"""
    assert 1 <= passes <= 5 and 0 <= zs <= 23 and 0 <= ls <= 16
    geom = np.asarray(geom, bool)
    I = np.where(geom[..., None], demodulate(rec, base), 0)
    out = []
    for k in range(1, passes + 1):
        I = one_pass(I, np.asarray(pid), np.asarray(z), geom, np.asarray(normal), k, zs, ls)
        out.append(store(I, rec, geom, base))
    return out


def denoise(rec, pid, z, geom, base, normal, passes, zs, ls):
    """the stored frame, uint32 ARGB [H, W]"""
    return frames(rec, pid, z, geom, base, normal, passes, zs, ls)[-1]


def unpack_normal(word):
    """the guide record's normal word (signed bytes x | y << 8 | z << 16) as int64 [..., 3]"""
    w = np.asarray(word).astype(np.uint32)
    return np.stack([((w >> np.uint32(s)) & np.uint32(0xFF)).astype(np.uint8).view(np.int8).astype(np.int64)
                     for s in (0, 8, 16)], -1)


def normals_f64(ptris, pid, geom):
    """the guide normal restated in float64 from the RT_REC_PTRIS records (float32 [P, 12]: v0 + pid, e1,
    e2): int64 [H, W, 3], 0 without geom or where the cross product has no finite length"""
    t = np.asarray(ptris, np.float64).reshape(-1, 12)
    p = np.where(geom, pid, 0)
    n = np.cross(t[p, 4:7], t[p, 8:11])
    ln = np.sqrt((n * n).sum(-1))
    good = geom & np.isfinite(ln) & (ln > 0)
    with np.errstate(all="ignore"):
        N = np.rint(n / ln[..., None] * 127.0)
    return np.where(good[..., None], N, 0).astype(np.int64)
