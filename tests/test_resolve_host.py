"""The material resolve's semantics on the CPU: the numpy fp32 restatement (tests/resolve_reference.py)
of Default.hlsl:50-116, run on the attributes of pbr_attributes_fill, is the host G-buffer fill bit for bit; the new
structs have the C compiler's layout; the new entry points validate arguments without a device. The device kernel is
held to the same restatement in tests/test_gpu_resolve.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import resolve_reference as R
from oracle import oracle as O
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd import scenes as S

CFG4 = S.CONFIGS[4].with_size(192, 128)


def test_restatement_on_config4_attributes_is_the_host_fill():
    planes, covered = S.fill_gbuffer_host(CFG4)
    attrs, mat = S.fill_attributes_host(CFG4)
    assert covered == 192 * 128 and (mat < 7).all()
    mats, texs = S.scene_materials(CFG4)
    assert len(mats) == 7
    present = sorted(set(mat.ravel().tolist()))
    has_metal = {bool(mats[m].flags & N.PBR_MAT_METALLIC_TEXTURE) for m in present}
    print("materials in the frame:", present)
    assert len(present) >= 3 and has_metal == {True, False}
    got, opacity, coverage = R.resolve(attrs, mat, mats, texs, R.POINT)
    for i, name in enumerate(N.PLANE_NAMES):
        assert O.bit_equal(got[i], planes[i]).all(), name
    assert (coverage == 1).all() and (opacity == 1.0).all()


@pytest.mark.parametrize("camera", [None, S.OVERVIEW_CAMERA], ids=["default", "overview"])
def test_reference_scene_attributes_match_the_fill(camera):
    cfg = S.REFERENCE_SCENE.with_size(160, 90)
    if camera is not None:
        cfg = cfg.with_camera(*camera)
    planes, cov = S.fill_gbuffer_host_coverage(cfg)
    attrs, mat = S.fill_attributes_host(cfg)
    assert 0 < cov.sum() < cov.size
    for c in range(3):
        assert O.bit_equal(attrs[c], planes[c]).all()
    assert np.array_equal(mat != N.PBR_MATERIAL_NONE, cov != 0)
    assert (mat[cov != 0] < 58).all()
    # background: the view direction passes through in the normal planes
    bg = cov == 0
    for c in range(3):
        assert O.bit_equal(attrs[3 + c][bg], planes[3 + c][bg]).all()
    mats, texs = S.scene_materials(cfg)
    assert len(mats) == 58
    got, _, coverage = R.resolve(attrs, mat, mats, texs, R.POINT)
    assert np.array_equal(coverage, cov)
    # untextured spheres (the 49 red ones and copper): constants only, so the resolve is the fill's
    plain = (mat < 49) | (mat == 50)
    assert plain.any()
    for i in (6, 7, 8, 9, 10, 12, 13, 14):
        assert O.bit_equal(got[i][plain], planes[i][plain]).all(), N.PLANE_NAMES[i]
    for i in range(15):  # and every background plane
        assert O.bit_equal(got[i][bg], planes[i][bg]).all(), N.PLANE_NAMES[i]


def test_restatement_filters_agree_at_texel_centres():
    """At a texel centre of a power-of-two texture (k + 0.5) / n * n - 0.5 is exactly k: the bilinear weights are
    exactly 0 and both filters return the decoded texel. (oracle.py exposes no environment bilinear to call on its
    own, so the restatement's linear filter is not compared with the oracle's here.)"""
    rng = np.random.default_rng(5)
    for (h, w, c) in ((64, 64, 1), (1, 1, 4), (2, 256, 3)):
        tex = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        ys, xs = [g.ravel() for g in np.meshgrid(np.arange(h), np.arange(w), indexing="ij")]
        u = (xs.astype(np.float32) + np.float32(0.5)) / np.float32(w)
        v = (ys.astype(np.float32) + np.float32(0.5)) / np.float32(h)
        nch = min(c, 3)
        p = R.sample(tex, u, v, R.POINT, nch)
        q = R.sample(tex, u, v, R.LINEAR, nch)
        for k in range(nch):
            direct = tex[ys, xs, k].astype(np.float32) / np.float32(255)
            assert O.bit_equal(p[k], direct).all() and O.bit_equal(q[k], direct).all(), (h, w, c, k)
    gray = R.sample(tex[:, :, 0], u, v, R.POINT, 3)  # a 1-channel texture read as .rgb replicates .r
    assert O.bit_equal(gray[1], gray[0]).all() and O.bit_equal(gray[2], gray[0]).all()


def test_wrap_index_matches_the_c_rule():
    f = np.array([0, 1, 4, 5, 6, -1, -5, -6, 1e9, -1e9, 2.5e9, -2.5e9, np.nan, np.inf, -np.inf], np.float32)
    got = R.wrap_index(f, 5)
    want = []
    for x in f.tolist():
        if x != x or x > 2.0e9 or x < -2.0e9:
            want.append(0)
        else:
            i = int(x)
            r = abs(i) % 5 * (1 if i >= 0 else -1)  # C's truncating %
            want.append(r + 5 if r < 0 else r)
    assert got.tolist() == want


NEW_STRUCTS = {"pbr_material": "MaterialDesc", "pbr_texture_desc": "TextureDesc",
               "pbr_attributes_soa": "AttributesSoA", "pbr_gbuffer_targets": "GBufferTargets"}


def test_new_struct_layouts_match_header(tmp_path):
    """As test_abi.test_struct_layouts_match_header, for the resolve's structs."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "pbr/pbr_shade.h"', "int main(void) {"]
    for cs, py in NEW_STRUCTS.items():
        lines.append(f'printf("{cs} size %zu\\n", sizeof({cs}));')
        for name, *_ in getattr(N, py)._fields_:
            lines.append(f'printf("{cs} {name} %zu\\n", offsetof({cs}, {name}));')
    lines += ['printf("enum none %d\\n", (int)PBR_MATERIAL_NONE);',
              'printf("enum filters %d\\n", PBR_FILTER_POINT * 10 + PBR_FILTER_LINEAR);',
              'printf("enum flags %d\\n", PBR_MAT_DIFFUSE_TEXTURE | PBR_MAT_SPECULAR_TEXTURE << 4 | '
              'PBR_MAT_METALLIC_TEXTURE << 8 | PBR_MAT_ROUGHNESS_TEXTURE << 12 | PBR_MAT_NORMAL_TEXTURE << 16 | '
              'PBR_MAT_ALPHA_TEST << 20);', "return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    inc = os.path.join(os.path.dirname(N.HEADER_PATH), "..")
    subprocess.run(["gcc", "-I", inc, str(src), "-o", exe], check=True)
    c_layout = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        cs, name, v = line.split()
        c_layout[(cs, name)] = int(v)
    for cs, py in NEW_STRUCTS.items():
        cls = getattr(N, py)
        assert c_layout[(cs, "size")] == ctypes.sizeof(cls), cs
        for name, *_ in cls._fields_:
            assert c_layout[(cs, name)] == getattr(cls, name).offset, f"{cs}.{name}"
    assert c_layout[("enum", "none")] == N.PBR_MATERIAL_NONE
    assert c_layout[("enum", "filters")] == N.PBR_FILTER_POINT * 10 + N.PBR_FILTER_LINEAR
    assert c_layout[("enum", "flags")] == (N.PBR_MAT_DIFFUSE_TEXTURE | N.PBR_MAT_SPECULAR_TEXTURE << 4 |
                                           N.PBR_MAT_METALLIC_TEXTURE << 8 | N.PBR_MAT_ROUGHNESS_TEXTURE << 12 |
                                           N.PBR_MAT_NORMAL_TEXTURE << 16 | N.PBR_MAT_ALPHA_TEST << 20)


def test_null_arguments_are_rejected_without_a_device():
    lib = N.lib()
    assert lib.pbr_set_materials(None, None, 0, None, 0, None) == -1
    assert lib.pbr_resolve_materials(None, None, None, 0, None) == -1
    assert lib.pbr_attributes_fill(None, 0, 0, None, None, 0, 1) == -1
    assert lib.pbr_abi_version() == 9  # the new entry points are additive


def test_attributes_fill_rejects_other_scenes_and_bad_rows():
    cfg = S.CONFIGS[2].with_size(16, 8)
    with pytest.raises(N.PbrError) as e:
        S.fill_attributes_host(cfg)
    assert e.value.status == N.PBR_ERR_UNSUPPORTED
    with pytest.raises(N.PbrError):
        S.fill_attributes_host(CFG4, 0, 129)


def test_attributes_fill_rows_are_independent():
    full, mat = S.fill_attributes_host(CFG4, n_threads=3)
    band, bmat = S.fill_attributes_host(CFG4, 61, 70, n_threads=1)
    assert O.bit_equal(full[:, 61:70], band).all() and np.array_equal(mat[61:70], bmat)
