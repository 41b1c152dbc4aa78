"""bench.py's measurement model on the CPU (no GPU): algorithmic bytes and FLOPs per pixel,
the compute-vs-HBM roof choice, the PMC lookup keyed by workload and mode, and the CPU baseline leg
(the reference's own shader build when present, else the C port) with its parity check."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT
import bench
from physically_based_renderer_amd import _native as N
from physically_based_renderer_amd import scenes as S


def test_bytes_per_pixel_model_and_reads():
    """SURVEY 8(d)'s algorithmic bytes (the roofline figure) beside what the kernel reads: 8(d) counts the AO plane of
    the north star's G-buffer, which the reference never reads and the kernel reads only with
    PBR_FLAG_APPLY_AO."""
    pc3 = S.scene_pass(S.CONFIGS[3])
    assert bench.bytes_per_pixel(pc3) == 64            # 12 planes + RGBA fp32 (8(d): configs 1-3, 5)
    assert bench.bytes_per_pixel(pc3, 4) == 52         # RGBA8 back buffer
    assert bench.bytes_read_per_pixel(pc3) == 60       # 11 planes read
    assert bench.bytes_read_per_pixel(pc3, 4) == 48
    pc3.flags = int(pc3.flags) | N.PBR_FLAG_APPLY_AO
    assert bench.bytes_read_per_pixel(pc3) == bench.bytes_per_pixel(pc3) == 64
    pc4 = S.scene_pass(S.CONFIGS[4])
    assert pc4.flags & N.PBR_FLAG_F0_PLANE
    assert bench.bytes_per_pixel(pc4) == 76            # + F0 plane (8(d): config 4)
    assert bench.bytes_read_per_pixel(pc4) == 72


def test_flops_per_pixel_and_the_roof():
    pc3 = S.scene_pass(S.CONFIGS[3])
    f3 = bench.flops_per_pixel(pc3)
    assert f3 == 27 + 20 + 91 * 64 + 87 == 5958
    # config 3 sits right of the ridge (compute roof), config 2 left of it (HBM roof)
    ridge = bench.FP32_PEAK_TFLOPS * 1e12 / (bench.HBM_PEAK_GBPS * 1e9)
    assert f3 / bench.bytes_per_pixel(pc3) > ridge
    pc2 = S.scene_pass(S.CONFIGS[2])
    assert bench.flops_per_pixel(pc2) / bench.bytes_per_pixel(pc2) < ridge
    # tiled culling counts the surviving lights, plus each light's range test once per culling tile
    pc4 = S.scene_pass(S.CONFIGS[4])
    f4 = bench.flops_per_pixel(pc4, lights_per_tile=5.0, tile_px=128)
    assert f4 == pytest.approx(47 + 91 * 5.0 + 9 * 256 / 128)


def test_pmc_lookup_is_keyed_by_workload_and_mode(tmp_path):
    summary = json.load(open(os.path.join(ROOT, "profiles", "pmc_summary.json")))
    head = N.kernel_sources_sha()
    for key in ("cfg3_3840x2160_64pt_ibl_chelsea", "cfg3_3840x2160_64pt_ibl_chelsea_faithful"):
        assert key in summary
        e = summary[key]
        traffic, busy, prov = bench.load_pmc(key, head)
        assert prov["kernel_sources_sha"] == head
        if e.get("kernel_sources_sha") == head:  # profiled at this revision of the kernels: quoted
            assert traffic == e["hbm_bytes_per_launch"] and 0.5 < busy <= 1.0 and "stale" not in prov
        else:  # a profile of other kernel sources is never quoted
            assert traffic is None and busy is None and prov["stale"]
        # HBM traffic within 15 % of the algorithmic bytes: no re-reads of the planes -- except where a profile
        # records the exact balanced kernel's second read of the pair after its loop (+44 B/px, 1.77x)
        assert 0.95 < e["traffic_over_algorithmic"] < (1.8 if e.get("pair_reread") else 1.15)
        # the committed kernel trace agrees with the bench's own events within 2 %
        kt = e["kernel_trace"]
        assert abs(kt["mean_ms_timed_steps"] - kt["bench_avg_launch_ms"]) / kt["bench_avg_launch_ms"] < 0.02
    assert bench.load_pmc("no_such_workload", head)[:2] == (None, None)
    # the stamp decides: the same entry quoted under this build's hash, refused under another
    e = dict(summary["cfg3_3840x2160_64pt_ibl_chelsea_faithful"])
    for sha, quoted in ((head, True), ("0" * 16, False)):
        e["kernel_sources_sha"] = sha
        p = tmp_path / f"s_{sha}.json"
        p.write_text(json.dumps({"w": e}))
        traffic, busy, prov = bench.load_pmc("w", head, str(p))
        assert (traffic == e["hbm_bytes_per_launch"]) if quoted else (traffic is None and prov["stale"])


def test_roofline_block_names_its_unit_and_the_profiled_box():
    """roofline: `bound` keeps the contract's vocabulary, `bound_unit` says which unit the roof is; `frac` from this
    run's events, `frac_profile` from the committed profile's kernel-trace mean and `launch_vs_profile` the ratio --
    only when the profile is of this build (stale: None)."""
    pc3 = S.scene_pass(S.CONFIGS[3])
    px = 3840 * 2160
    fpp, bpp = bench.flops_per_pixel(pc3), bench.bytes_per_pixel(pc3)
    stats = {"geometry_pixels": px, "light_terms": 32 * px, "backface_tests": 64 * px, "cull_tiles": 0,
             "exact_pixels": 0}
    prov = {"profile": "p", "kernel_sources_sha": "a", "profile_kernel_sources_sha": "a", "profile_kernel_mean_ms": 0.85}
    r = bench.roofline_block(fpp, 3560.0, bpp, 60, px, 0.816e-3, 0.815, 5.16e8, 0.886, prov, "k", stats)
    assert r["bound"] == "mfma" and r["bound_unit"] == "valu" and r["unit"] == "TFLOP/s"
    assert r["frac"] == pytest.approx(fpp * px / 0.816e-3 / 1e12 / bench.FP32_PEAK_TFLOPS, abs=1e-4)
    assert r["frac_profile"] == pytest.approx(fpp * px / 0.85e-3 / 1e12 / bench.FP32_PEAK_TFLOPS, abs=1e-4)
    assert r["launch_vs_profile"] == pytest.approx(0.816 / 0.85, abs=1e-4)
    r = bench.roofline_block(fpp, 3560.0, bpp, 60, px, 0.816e-3, 0.815, None, None, {**prov, "stale": True}, "k", stats)
    assert r["frac_profile"] is None and r["launch_vs_profile"] is None
    pc2 = S.scene_pass(S.CONFIGS[2])
    f2, b2 = bench.flops_per_pixel(pc2), bench.bytes_per_pixel(pc2)
    r = bench.roofline_block(f2, f2, b2, 60, 1920 * 1080, 51e-6, 0.051, None, None, prov, "k", stats)
    assert r["bound"] == r["bound_unit"] == "hbm" and r["unit"] == "GB/s"
    assert r["frac_profile"] == pytest.approx(b2 * 1920 * 1080 / 0.85e-3 / 1e9 / bench.HBM_PEAK_GBPS, abs=1e-5)
    # the committed summary carries the profiled box's kernel mean for the headline workload
    e = json.load(open(os.path.join(ROOT, "profiles", "pmc_summary.json")))["cfg3_3840x2160_64pt_ibl_chelsea_faithful"]
    _, _, p = bench.load_pmc("cfg3_3840x2160_64pt_ibl_chelsea_faithful", e["kernel_sources_sha"])
    assert p["profile_kernel_mean_ms"] == round(e["kernel_trace"]["mean_ms_timed_steps"], 4)
    assert bench.LINE_SCHEMA == 6


def test_executed_flops_count_only_evaluated_terms():
    """frac_executed's model: per geometry pixel the fixed part, 91 / 74 FLOP per evaluated point / directional
    term, 8 per back-face test of the balanced lists, the range tests of culled passes."""
    pc3 = S.scene_pass(S.CONFIGS[3])
    px = 1000
    full = {"geometry_pixels": px, "light_terms": 64 * px, "backface_tests": 0, "culled": 0, "cull_tiles": 0}
    assert bench.executed_flops_per_pixel(pc3, full, px) == bench.flops_per_pixel(pc3) == 5958
    half = dict(full, light_terms=32 * px, backface_tests=64 * px)  # balanced: half the terms live
    assert bench.executed_flops_per_pixel(pc3, half, px) == 27 + 20 + 87 + 91 * 32 + 8 * 64
    pc4 = S.scene_pass(S.CONFIGS[4])
    culled = {"geometry_pixels": px, "light_terms": 5 * px, "backface_tests": 0, "culled": 1, "cull_tiles": 8}
    assert bench.executed_flops_per_pixel(pc4, culled, px) == pytest.approx(47 + 91 * 5 + 9 * 256 * 8 / px, abs=0.01)


@pytest.mark.parametrize("kind", ["auto", "port"])
def test_cpu_baseline_leg_checks_parity(kind):
    from oracle import oracle as O

    cfg = S.CONFIGS[3].with_size(256, 16)
    planes, _ = S.fill_gbuffer_host(cfg)
    pc = S.scene_pass(cfg)
    env = S.env_map()
    ops = O.OraclePass(eye=tuple(pc.eye_pos_w), ambient=tuple(pc.ambient_light), fresnel_r0=tuple(pc.fresnel_r0),
                       opacity=pc.opacity, n_point=pc.num_point_lights, ambient_mode=pc.ambient_mode)
    frame = O.shade(list(planes), ops, pc.light_array(), env, n_threads=4)  # stands in for the GPU frame
    cpu, parity, (step, ref) = bench.cpu_baseline(cfg, planes, pc, env, frame, 0, kind)
    assert cpu["kind"] == ("reference" if kind == "auto" and O.ref_available() else "port")
    assert cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["single_thread_value"] > 0
    # every core of the affinity mask (capped only by a cgroup quota), with the host counts stated
    hc = cpu["host_cpus"]
    assert cpu["cores"] == hc["used"] and hc["affinity"] == len(os.sched_getaffinity(0))
    assert hc["os_cpu_count"] == os.cpu_count() and hc["used"] <= hc["affinity"]
    assert parity["parity_max_rel"] == 0.0 and parity["parity_bit_exact_frac"] == 1.0 and step == 1
    assert np.array_equal(ref.view(np.uint32), frame.view(np.uint32))


def test_cpu_baseline_rgba8_and_gathered_parity():
    """RGBA8 output (config 5's presented frame): the CPU leg shades in the same format and compares codes;
    the N > 1 check refills the sampled rows of every band and compares the assembled frame."""
    from oracle import oracle as O

    cfg = S.CONFIGS[5].with_size(128, 48)
    pc = S.scene_pass(cfg)
    env = S.env_map()
    planes, _ = S.fill_gbuffer_host(cfg)
    frame8 = O.shade_frame(list(planes), bench.oracle_pass_of(pc), pc.light_array(), env, None, None,
                           O.OUTPUT_RGBA8, n_threads=4)
    cpu, parity, (step, ref) = bench.cpu_baseline(cfg, planes, pc, env, frame8, 0, "port", rgba8=True)
    assert ref.dtype == np.uint8 and parity == {"parity_max_code_diff": 0, "parity_bit_exact_frac": 1.0}
    bad = frame8.copy()
    bad[20, 5, 1] ^= 1
    p = bench.gathered_parity(cfg, pc, env, bad, 3, 4, rgba8=True)
    assert p["rows_checked"] == 12 and p["parity_max_code_diff"] == 1  # band 1 = rows 16-31, sampled at 16, 20, 24, 28
    frame32 = O.shade(list(planes), bench.oracle_pass_of(pc), pc.light_array(), env, n_threads=4)
    p = bench.gathered_parity(cfg, pc, env, frame32, 3, 4, rgba8=False)
    assert p["parity_max_rel"] == 0.0 and p["parity_bit_exact_frac"] == 1.0


def test_host_cpu_budget_reads_the_quota():
    b = bench.host_cpu_budget()
    assert b["used"] >= 1 and b["affinity"] >= b["used"]


def test_bench_refuses_to_publish_a_wrong_frame(capsys):
    """The north-star bar is enforced, not just reported: a bench line whose frame check misses 1e-5 relative (or
    whose NaN pattern differs, or an RGBA8 code off by more than 1, or a failed gather checksum) is not printed on
    stdout and main() exits with EXIT_PARITY -- the driver then records a failed run, never a throughput."""
    from oracle import oracle as O

    cfg = S.CONFIGS[3].with_size(128, 8)
    planes, _ = S.fill_gbuffer_host(cfg)
    pc = S.scene_pass(cfg)
    env = S.env_map()
    frame = O.shade(list(planes), bench.oracle_pass_of(pc), pc.light_array(), env, n_threads=4)
    base = {"metric": bench.METRIC, "value": 1.0}

    def run(gpu_frame):
        _, parity, _ = bench.cpu_baseline(cfg, planes, pc, env, gpu_frame, 0, "port")
        rc = bench.emit_line({**base, **parity})
        return rc, capsys.readouterr()

    rc, out = run(frame)
    assert rc == 0 and json.loads(out.out)["parity_ok"] is True
    ok_within = frame.copy()
    ok_within[3, 7, 1] *= 1 + 5e-6  # inside the bar
    rc, out = run(ok_within)
    assert rc == 0 and json.loads(out.out)["parity_ok"] is True
    for breach in ("rel", "nan", "lost_nan"):
        bad = frame.copy()
        if breach == "rel":
            bad[3, 7, 1] *= 1 + 2e-5
        elif breach == "nan":
            bad[0, 0, 0] = np.nan
        else:
            bad = bad[..., :3] * 0 + np.nan  # NaN everywhere the reference has numbers
            bad = np.concatenate([bad, frame[..., 3:]], axis=-1).astype(np.float32)
        rc, out = run(bad)
        assert rc == bench.EXIT_PARITY, breach
        assert out.out == "" and "PARITY FAILURE" in out.err
    # the other checks a line can carry
    for line in ({"parity_max_code_diff": 2}, {"gathered_frame_parity": {"parity_max_rel": 3e-5}},
                 {"parity_max_rel": 0.0, "exact_mode": {"parity_max_rel": float("inf")}},
                 {"gathered_frame_parity": {"parity_max_code_diff": 1}, "gather_checksums_match": False}):
        assert bench.parity_failures(line), line
        assert bench.emit_line({**base, **line}) == bench.EXIT_PARITY
        assert capsys.readouterr().out == ""
    assert bench.parity_failures({"parity_max_code_diff": 1, "gathered_frame_parity": {"parity_max_rel": 1e-5}}) == []
    # a line without any check (--no-cpu-baseline) is printed and says so
    assert bench.emit_line(dict(base)) == 0
    assert json.loads(capsys.readouterr().out)["parity_checked"] is False


def test_dump_outputs_writes_float32_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs: a small output is written whole in its own shape, RGBA8 codes as float32 values; an output
    over its share of the budget as the same seeded pixel sample on every call, so two builds can be compared."""
    import torch

    assert bench.DUMP_BUDGET_BYTES + 2 * 4096 <= 64 * 1000 * 1000  # the files' headers included
    small = torch.arange(6 * 5 * 4, dtype=torch.float32).reshape(6, 5, 4)
    small[2, 3, 1] = float("nan")
    codes = (torch.arange(3 * 7 * 4) % 256).to(torch.uint8).reshape(3, 7, 4)
    shapes = bench.dump_outputs(str(tmp_path / "a"), {"frame": small, "gathered_frame": codes})
    assert shapes == {"frame": [6, 5, 4], "gathered_frame": [3, 7, 4]}
    got = np.load(tmp_path / "a" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), small.numpy().view(np.uint32))
    got8 = np.load(tmp_path / "a" / "gathered_frame.npy")
    assert got8.dtype == np.float32 and np.array_equal(got8, codes.numpy().astype(np.float32))
    # over the budget: 1000 pixels, room for 100 per file
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 100 * 16)
    big = torch.arange(1000 * 4, dtype=torch.float32).reshape(25, 40, 4)
    for d in ("b", "c"):
        assert bench.dump_outputs(str(tmp_path / d), {"frame": big, "gathered_frame": codes}) == {
            "frame": [100, 4], "gathered_frame": [3, 7, 4]}
    b, c = np.load(tmp_path / "b" / "frame.npy"), np.load(tmp_path / "c" / "frame.npy")
    assert np.array_equal(b, c) and b.nbytes + got8.nbytes <= bench.DUMP_BUDGET_BYTES
    px = (b[:, 0] // 4).astype(int)  # channel 0 of pixel k is 4k: the sampled pixels, ascending and distinct
    assert np.all(np.diff(px) > 0) and np.array_equal(b, big.reshape(-1, 4).numpy()[px])


def test_scale_anchor_ramps_the_clock_before_timing(monkeypatch):
    """band_anchor runs the same untimed clock ramp as the headline (--ramp-ms) before its warm-up and timed
    steps, and reports it; the anchor is then comparable with the ramped per-N values it divides."""
    import argparse
    import types

    calls = []
    monkeypatch.setattr(bench.torch.cuda, "synchronize", lambda *a, **k: None)

    class Ctx:
        def shade_frame(self, gb, o, fmt=None, stream=None):
            calls.append("shade")

    def fake_steps(shade_into, outs, stream, warmup, steps, *a, **k):
        calls.append("timed")
        return 0.01, [1.0] * steps

    monkeypatch.setattr(bench, "shade_steps", fake_steps)
    args = argparse.Namespace(rows_per_rank=8, mode="faithful", warmup=1, steps=4, ramp_ms=5.0)
    resident = (types.SimpleNamespace(), [object(), object()])
    a = bench.band_anchor(Ctx(), args, 1, None, None, resident)
    assert a["clock_ramp"]["launches"] >= 8 and a["clock_ramp"]["ms"] >= 5.0
    assert calls.index("timed") == len(calls) - 1 and calls[:-1] == ["shade"] * a["clock_ramp"]["launches"]
    calls.clear()
    a = bench.band_anchor(Ctx(), argparse.Namespace(**{**vars(args), "ramp_ms": 0.0}), 1, None, None, resident)
    assert a["clock_ramp"] == {"ms": 0.0, "launches": 0} and calls == ["timed"]
