"""mi_phase_sort against what a caller does today for the same order, on one box.

    python tools/probes/phase_sort_probe.py [--sizes 4096,65536,1048576] [--reps 21] [--out FILE.md]

Per size: n rows, all visible, all in one class (so the phase has n items), translations uniform in a +-100 box, a rotated camera.
  device   mi_phase_sort alone, event-timed on the context's stream (median after 3 warm-up calls)
  dev+dl   mi_phase_sort + mi_phase_sort_download of rows and distances, wall clock -- a caller that wants the order on the host
  host     mi_download_visible_entities + gather of the translations from a host copy of the GlobalTransforms + the f32 dot +
           np.argsort(kind="stable") on the mapped key, wall clock
The host figure is numpy's: its stable argsort of u32 keys is a radix sort, as radsort is."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import bevy_amd as B  # noqa: E402


def median_of(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    return float(np.median([fn() for _ in range(reps)]))


def run(n, reps):
    rng = np.random.default_rng(n)
    g = np.zeros((n, 12), np.float32)
    g[:, 0] = g[:, 4] = g[:, 8] = 1
    g[:, 9:12] = rng.uniform(-100, 100, (n, 3)).astype(np.float32)
    row2 = np.array([0.48, -0.36, 0.8, -12.5], np.float32)
    with B.Context() as ctx:
        ctx.resize(n)
        ctx.upload_global_transforms(g.reshape(-1))
        ctx.upload_bounds(np.zeros(3 * n, np.float32), np.zeros(3 * n, np.float32),
                          np.full(n, B.FLAG_INHERITED_VISIBLE | B.FLAG_NO_FRUSTUM_CULLING, np.uint8))
        ctx.cull(np.tile(np.array([0, 0, 0, 1], np.float32), 6), flags=B.CULL_BEGIN_FRAME | B.CULL_END_FRAME)
        ctx.synchronize()

        def device():
            ctx.timer_begin()
            ctx._ck(ctx._lib.mi_phase_sort(ctx._h, 0, 0, row2.ctypes.data_as(B.api.C.POINTER(B.api.C.c_float)), 0))
            return 1e3 * ctx.timer_end()

        def device_and_download():
            t0 = time.perf_counter()
            got = ctx.phase_sort(0, 0, row2)
            assert len(got["rows"]) == n
            return 1e6 * (time.perf_counter() - t0)

        def host():
            t0 = time.perf_counter()
            _, rows = ctx.download_visible_entities(0, 0)
            t = g[rows, 9:12]
            d = (row2[0] * t[:, 0] + row2[2] * t[:, 2]) + (row2[1] * t[:, 1] + row2[3]) + np.float32(0)
            bits = d.view(np.uint32)
            order = np.argsort(bits ^ np.where(bits >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)), kind="stable")
            host.rows = rows[order]
            return 1e6 * (time.perf_counter() - t0)

        res = dict(n=n, device_us=median_of(device, reps), dev_dl_us=median_of(device_and_download, reps), host_us=median_of(host, reps))
        assert np.array_equal(ctx.phase_sort(0, 0, row2)["rows"], host.rows)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,65536,1048576")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = ["| items | mi_phase_sort (device, µs) | + download (wall, µs) | host path (wall, µs) | bytes per pass (MB) | GB/s over 4 passes |",
             "|---|---|---|---|---|---|"]
    for n in [int(s) for s in a.sizes.split(",")]:
        r = run(n, a.reps)
        mb = 24e-6 * n  # a pass of the tiled form reads the 8-byte pairs twice (histogram, scatter) and writes them once
        lines.append(f"| {n} | {r['device_us']:.1f} | {r['dev_dl_us']:.0f} | {r['host_us']:.0f} | {mb:.2f} | {4 * 24e-3 * n / r['device_us']:.0f} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
