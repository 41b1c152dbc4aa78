"""The anisotropic resolve (pbr_resolve_materials_aniso; DESIGN.md §11, "Anisotropic filter") restated in numpy on top
of tests/resolve_mip_reference.py (footprints, chains, the level of detail from r2 on) and tests/resolve_reference.py
(the bilinear and everything outside the five maps): fp32 with one numpy operation per operation of the rule, so every
+, -, *, / rounds once. A helper, not a test: tests/test_resolve_aniso_host.py holds it to the rule,
tests/test_gpu_resolve_aniso.py holds the device kernel to it bit for bit."""
import numpy as np

import resolve_mip_reference as RM
import resolve_reference as R
from physically_based_renderer_amd import _native as N

F = np.float32
MAX_ANISOTROPY = 16  # D3D12's range is 1 .. 16


def footprint_axes(dudx, dvdx, dudy, dvdy, w, h):
    """(pmax2, pmin2, du, dv) of a texture of w x h texels: the squared texel lengths of the longer and the shorter
    screen-axis footprint, and the longer one's UV step. ymajor = ry > rx is false for NaN."""
    with np.errstate(all="ignore"):
        ax, ay = dudx * F(w), dvdx * F(h)
        bx, by = dudy * F(w), dvdy * F(h)
        rx = ax * ax + ay * ay
        ry = bx * bx + by * by
        ymajor = ry > rx
        pmax2 = np.where(ymajor, ry, rx)
        pmin2 = np.where(ymajor, rx, ry)
        du = np.where(ymajor, dudy, dudx)
        dv = np.where(ymajor, dvdy, dvdx)
    return pmax2, pmin2, du, dv


def tap_count(pmax2, pmin2, max_anisotropy):
    """N: 1, then for k = 1 .. M-1 ascending N = k + 1 where pmax2 > (float)(k k) * pmin2."""
    pmax2, pmin2 = np.asarray(pmax2, F), np.asarray(pmin2, F)
    n = np.ones(pmax2.shape, np.int32)
    with np.errstate(all="ignore"):
        for k in range(1, int(max_anisotropy)):
            n = np.where(pmax2 > F(k * k) * pmin2, np.int32(k + 1), n)
    return n


def level_r2(pmax2, n):
    """r2 = N > 1 ? pmax2 / (float)(N N) : pmax2."""
    with np.errstate(all="ignore"):
        return np.where(n > 1, pmax2 / (n * n).astype(F), pmax2).astype(F)


def lod_from_r2(r2, n_levels, lod_bias):
    """(l0, l1, f, lod): the operations of resolve_mip_reference.lod from r2 on (tests/test_resolve_aniso_host.py holds
    the two to each other)."""
    with np.errstate(all="ignore"):
        b = r2.view(np.uint32)
        e = (b >> 23).astype(np.int32) - 127
        m = b & np.uint32(0x7FFFFF)
        l2 = e.astype(F) + m.astype(F) * F(2.0 ** -23)
        base = np.where(r2 > F(1.0), F(0.5) * l2, F(0.0)).astype(F)
        lv = base + F(lod_bias)
        lv = np.where(lv < F(0.0), F(0.0), lv)
        last = F(n_levels - 1)
        lv = np.where(lv > last, last, lv).astype(F)
        l0 = np.floor(lv).astype(np.int32)
        f = lv - l0.astype(F)
        l1 = np.minimum(l0 + 1, n_levels - 1)
    return l0, l1, f, lv


def tap_offsets(n):
    """t_i = (float)(2 i + 1 - N) / (float)(2 N) for i = 0 .. N-1, a float32 array of N values."""
    i = np.arange(n, dtype=np.int32)
    return (2 * i + 1 - n).astype(F) / F(2 * n)


def lod(dudx, dvdx, dudy, dvdy, w, h, n_levels, lod_bias, max_anisotropy):
    """(N, l0, l1, f, lod) of a texture of w x h texels and n_levels levels."""
    pmax2, pmin2, _, _ = footprint_axes(dudx, dvdx, dudy, dvdy, w, h)
    n = tap_count(pmax2, pmin2, max_anisotropy)
    return (n,) + lod_from_r2(level_r2(pmax2, n), n_levels, lod_bias)


def sample(chain, u, v, d, lod_bias, max_anisotropy, nch):
    """nch channels of the chain (resolve_mip_reference.build_mips) at float32 (u, v) (1-D) with footprints d."""
    h, w = chain[0].shape[0], chain[0].shape[1]
    pmax2, pmin2, du, dv = footprint_axes(*d, w, h)
    n = tap_count(pmax2, pmin2, max_anisotropy)
    l0, l1, f, _ = lod_from_r2(level_r2(pmax2, n), len(chain), lod_bias)
    c0 = [np.empty(u.shape, F) for _ in range(nch)]
    c1 = [np.empty(u.shape, F) for _ in range(nch)]
    with np.errstate(all="ignore"):
        for count in np.unique(n):
            of_count = n == count
            taps = tap_offsets(int(count))
            for lvl, tex in enumerate(chain):
                for which, dst in ((l0, c0), (l1, c1)):
                    sel = of_count & (which == lvl)
                    if not sel.any():
                        continue
                    if count == 1:
                        s = R.sample(tex, u[sel], v[sel], R.LINEAR, nch)
                    else:
                        s = None
                        for t in taps:
                            ui = u[sel] + t * du[sel]  # a product, then a sum
                            vi = v[sel] + t * dv[sel]
                            got = R.sample(tex, ui, vi, R.LINEAR, nch)
                            s = got if s is None else [s[c] + got[c] for c in range(nch)]
                        s = [s[c] / F(count) for c in range(nch)]
                    for c in range(nch):
                        dst[c][sel] = s[c]
        return [R.lerp(c0[c], c1[c], f) for c in range(nch)]


def resolve_aniso(attrs, material, materials, textures, max_anisotropy=8, lod_bias=0.0, chains=None):
    """resolve_mip_reference.resolve_mip with the anisotropic filter on the five material maps; the ALPHA_TEST opacity
    stays the level-0 point tap. `chains`: build_mips of every texture, when the caller has them already."""
    assert 1 <= int(max_anisotropy) <= MAX_ANISOTROPY
    attrs = np.asarray(attrs, F)
    ids = np.asarray(material).astype(np.int64) & 0xFFFF
    if chains is None:
        chains = [RM.build_mips(t) for t in textures]
    d_full = RM.footprints(attrs[12], attrs[13], ids)
    # everything but the five maps is resolve_reference's: start from its point result and replace the sampled planes
    planes, opacity, coverage = R.resolve(attrs, ids, materials, textures, R.POINT)
    with np.errstate(all="ignore"):
        for mid, m in enumerate(materials):
            sel = ids == mid
            if not sel.any():
                continue
            a = attrs[:, sel]
            d = [x[sel] for x in d_full]
            u, v = a[12], a[13]
            fl, tex = int(m.flags), [int(t) for t in m.tex]
            n = u.shape[0]
            const = lambda val: np.full(n, F(val), F)
            smp = lambda slot, nch: sample(chains[tex[slot]], u, v, d, lod_bias, max_anisotropy, nch)
            alb = smp(0, 3) if fl & N.PBR_MAT_DIFFUSE_TEXTURE else [const(c) for c in m.diffuse_albedo]
            metal = smp(2, 1)[0] if fl & N.PBR_MAT_METALLIC_TEXTURE else const(m.metallic)
            if fl & N.PBR_MAT_SPECULAR_TEXTURE:
                f0 = smp(1, 3)
            else:
                f0 = [R.lerp(const(m.fresnel_r0[c]), alb[c], metal) for c in range(3)]
            rough = smp(3, 1)[0] if fl & N.PBR_MAT_ROUGHNESS_TEXTURE else const(m.roughness)
            if fl & N.PBR_MAT_NORMAL_TEXTURE:
                nx, ny, nz = a[3], a[4], a[5]
                length = np.sqrt((nx * nx + ny * ny) + nz * nz)
                nw = [nx / length, ny / length, nz / length]
                s = smp(4, 3)
                nt = [F(2.0) * s[c] - F(1.0) for c in range(3)]
                nrm = [(nt[0] * a[6 + c] + nt[1] * a[9 + c]) + nt[2] * nw[c] for c in range(3)]
                for c in range(3):
                    planes[3 + c][sel] = nrm[c]
            for c in range(3):
                planes[6 + c][sel] = alb[c]
                planes[12 + c][sel] = f0[c]
            planes[9][sel] = metal
            planes[10][sel] = rough
    return planes, opacity, coverage
