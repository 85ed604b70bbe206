"""The scale part of the row summary (RowSummary, kernels.h): waves of 64 rows whose Transform.scale agrees bit for bit take it from
the summary in the all-rows frame kernels instead of reading the column.

Every frame here is compared byte for byte (GlobalTransform, ViewVisibility) against the CPU oracle and against the same calls on
a second context with the summary switched off (debug_set_row_summary(1): every row reads its own columns).  The debug query
(debug_scale_summary_uniform_waves) says which waves are flagged, so that none of this passes with the fast path never taken --
and, above all, that every way of writing the scale column brings the summary up to date again (an under-touched summary is the one
way this feature can produce wrong results)."""
import numpy as np
import pytest

import bevy_amd as B
from bevy_amd import api, workloads as W
import oracle_lib as O

pytestmark = pytest.mark.gpu
F = np.float32
SCALE = (2.0, 0.5, -3.0)  # not ONE: a path that assumes it fails
ODD = (1.5, 0.5, -3.0)
SMALL_UPLOAD_ROWS = 4096  # kernels.h


@pytest.fixture
def pair():
    """(the context under test, the same with the row summary off)"""
    a, b = api.Context(0), api.Context(0)
    a.debug_set_row_summary(0)  # (whatever MI_TEST_ROW_SUMMARY says: these tests are about the summary)
    b.debug_set_row_summary(1)
    yield a, b
    a.close()
    b.close()


def frusta_for(n_views):
    cfv = api.perspective_clip_from_view(W.CAMERA_FOV, W.CAMERA_ASPECT, W.CAMERA_NEAR)
    cams = [W.many_cubes_camera(0), W.many_cubes_camera(5, yaw=1.5), W.many_cubes_camera(9, yaw=3.1), W.many_cubes_camera(3, yaw=4.4)]
    return np.concatenate([api.compute_frustum(cfv, cam, W.CAMERA_FAR) for cam in cams[:n_views]])


def scene(n, scale=SCALE):
    sc = W.many_cubes(n, radius=5.0 if n < 1000 else 60.0)
    sc["scale"] = np.tile(np.array(scale, F), n)
    return sc


def upload(ctx, sc):
    ctx.resize(sc["n"])
    ctx.upload_transforms(sc["translation"], sc["rotation"], sc["scale"])
    ctx.upload_bounds(sc["aabb_center"], sc["aabb_half"], sc["flags"], sc["layers"])


class Carried:
    """The oracle's ViewVisibility from frame to frame."""
    def __init__(self, n):
        self.vv = np.zeros(n, np.uint8)


def check_frame(pair, sc, carried, n_views=1, what=""):
    """One all-rows frame on both contexts; both against the oracle, byte for byte."""
    fr = frusta_for(n_views)
    g_exp, vv_exp, _, _ = O.full_frame(sc["translation"], sc["rotation"], sc["scale"], sc["aabb_center"], sc["aabb_half"], sc["flags"],
                                       sc["layers"], carried.vv, fr)
    for name, ctx in zip(("summary", "plain columns"), pair):
        ctx.propagate_and_cull(fr)
        ctx.visibility_end_frame()
        g, _ = ctx.download_global_transforms()
        vv, _ = ctx.download_view_visibility()
        assert g.tobytes() == g_exp.tobytes(), f"{what}: GlobalTransform ({name}) against the oracle"
        assert vv.tobytes() == vv_exp.tobytes(), f"{what}: ViewVisibility ({name}) against the oracle"
    carried.vv = vv_exp


def waves(n):
    return (n + 63) // 64


def assert_flags(ctx, n, not_uniform=(), what=""):
    count, flags, _ = ctx.debug_scale_summary_uniform_waves()
    exp = np.ones(waves(n), np.uint8)
    exp[list(not_uniform)] = 0
    assert flags.tobytes() == exp.tobytes(), f"{what}: waves flagged uniform {np.nonzero(flags)[0].tolist()}, expected all but {list(not_uniform)}"
    assert count == int(exp.sum())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 50_003])
def test_uniform_scale_every_wave_is_summarised(pair, n):
    sc = scene(n)
    for ctx in pair:
        upload(ctx, sc)
    carried = Carried(n)
    check_frame(pair, sc, carried, what=f"n {n}")
    assert_flags(pair[0], n)
    assert pair[1].debug_scale_summary_uniform_waves()[0] == 0  # switched off: nothing is derived
    check_frame(pair, sc, carried, what=f"n {n}, second frame")


@pytest.mark.parametrize("n,row,base,odd", [
    (257, 64, SCALE, ODD),                               # lane 0
    (257, 127, SCALE, ODD),                              # lane 63
    (200, 199, SCALE, ODD),                              # the last live row of a partial final wave
    (257, 70, (2.0, 0.0, -3.0), (2.0, -0.0, -3.0)),      # -0.0 against 0.0 in one component: not the same bits
], ids=["lane0", "lane63", "last_live_row", "negative_zero"])
def test_one_row_differs(pair, n, row, base, odd):
    sc = scene(n, base)
    sc["scale"][3 * row:3 * row + 3] = np.array(odd, F)
    for ctx in pair:
        upload(ctx, sc)
    check_frame(pair, sc, Carried(n), what=f"row {row}")
    assert_flags(pair[0], n, not_uniform=[row >> 6], what=f"row {row}")


def _rows_of(sc, rows):
    rows = np.asarray(rows)
    return (sc["translation"].reshape(-1, 3)[rows].reshape(-1), sc["rotation"].reshape(-1, 4)[rows].reshape(-1), sc["scale"].reshape(-1, 3)[rows].reshape(-1))


def _window(ctx, sc, rows, dense, components="trs"):
    rows = np.asarray(rows, np.uint32)
    k = len(rows)
    w, wrows, wt, wr, ws = ctx.map_upload_window(k, dense=dense, components=components)
    t, r, s = _rows_of(sc, rows)
    if wrows is not None:
        wrows[:] = rows
    for dst, src in ((wt, t), (wr, r), (ws, s)):
        if dst is not None:
            dst[:] = src
    ctx.commit_upload_window(w, k, first_row=int(rows[0]) if dense else 0)


def write_scale(ctx, sc, row, path):
    """Hands the scene's current Transform of `row` (and of whatever else the path carries) to the context."""
    n = sc["n"]
    near = np.arange(max(row - 2, 0), min(row + 3, n))
    if path == "dense_small":
        ctx.upload_transforms(*_rows_of(sc, near), first_row=int(near[0]))
    elif path == "dense_large":
        assert n > SMALL_UPLOAD_ROWS
        ctx.upload_transforms(sc["translation"], sc["rotation"], sc["scale"])
    elif path == "indexed":
        ctx.upload_transforms_indexed(np.array([row], np.uint32), *_rows_of(sc, [row]))
    elif path == "window_dense":
        _window(ctx, sc, near, dense=True)
    elif path == "window_dense_pieces":  # the whole table in one dense window, sent in pieces on the upload stream
        ctx.debug_set_chunked_frames(2)
        _window(ctx, sc, np.arange(n), dense=True)
    elif path == "window_indexed":
        _window(ctx, sc, [5, row, n - 3], dense=False)
    elif path == "window_indexed_descending":
        _window(ctx, sc, [n - 3, row, 5], dense=False)
    elif path == "window_indexed_unordered":
        _window(ctx, sc, [row, 5, n - 3], dense=False)
    elif path == "window_scale_only":
        _window(ctx, sc, [row], dense=False, components="s")
    else:
        raise AssertionError(path)


@pytest.mark.parametrize("path", ["dense_small", "dense_large", "indexed", "window_dense", "window_dense_pieces", "window_indexed",
                                  "window_indexed_descending", "window_indexed_unordered", "window_scale_only"])
def test_every_writer_of_scale_refreshes_the_summary(pair, path):
    n, row = SMALL_UPLOAD_ROWS + 1100, 4500
    sc = scene(n)
    for ctx in pair:
        upload(ctx, sc)
    carried = Carried(n)
    check_frame(pair, sc, carried, what="uniform")
    assert_flags(pair[0], n)
    for value, not_uniform in ((ODD, [row >> 6]), (SCALE, [])):  # one row's scale changes through the path, then goes back
        sc["scale"][3 * row:3 * row + 3] = np.array(value, F)
        for ctx in pair:
            write_scale(ctx, sc, row, path)
        check_frame(pair, sc, carried, what=f"{path}, scale of row {row} = {value}")
        assert_flags(pair[0], n, not_uniform, what=f"{path}, scale of row {row} = {value}")


@pytest.mark.parametrize("grow", [100, 3000], ids=["inside_the_allocation", "reallocated"])
def test_resize_then_upload_of_the_new_rows(pair, grow):
    n0, n1 = 5000, 5000 + grow
    full = scene(n1)
    first = {k: (n0 if k == "n" else v[:len(v) // n1 * n0]) for k, v in full.items()}
    for ctx in pair:
        upload(ctx, first)
    carried = Carried(n0)
    check_frame(pair, first, carried, what="before the resize")
    assert_flags(pair[0], n0)
    carried.vv = np.concatenate([carried.vv, np.zeros(grow, np.uint8)])  # (new rows start with ViewVisibility 0)
    new = np.arange(n0, n1)
    for ctx in pair:
        ctx.resize(n1)
        ctx.upload_bounds(full["aabb_center"][3 * n0:], full["aabb_half"][3 * n0:], full["flags"][n0:], full["layers"][n0:], first_row=n0)
    assert n0 % 64  # (row n0 shares its wave with rows of the old scale: that wave is mixed, the waves behind it uniform in the new one)
    for value, not_uniform in ((ODD, [n0 >> 6]), (SCALE, [])):
        full["scale"][3 * n0:] = np.tile(np.array(value, F), grow)
        for ctx in pair:
            ctx.upload_transforms(*_rows_of(full, new), first_row=n0)
        check_frame(pair, full, carried, what=f"grown by {grow}, new rows' scale {value}")
        assert_flags(pair[0], n1, not_uniform, what=f"grown by {grow}, new rows' scale {value}")
    for ctx in pair:  # ... and shrinks again: the wave the new end lies in is summarised over fewer rows
        ctx.resize(n0 - 37)
    small = {k: (n0 - 37 if k == "n" else v[:len(v) // n1 * (n0 - 37)]) for k, v in full.items()}
    carried.vv = carried.vv[:n0 - 37]
    check_frame(pair, small, carried, what="shrunk")
    assert_flags(pair[0], n0 - 37, what="shrunk")


def test_a_window_without_scale_leaves_the_part_alone(pair):
    n = 5200
    sc = scene(n)
    for ctx in pair:
        upload(ctx, sc)
    carried = Carried(n)
    check_frame(pair, sc, carried, what="uniform")
    count0, _, launches0 = pair[0].debug_scale_summary_uniform_waves()
    assert count0 == waves(n) and launches0 >= 1
    rows = np.arange(100, 4000, 7)
    q = W.random_unit_quats(11, len(rows)).astype(F)
    sc["rotation"].reshape(-1, 4)[rows] = q
    sc["translation"].reshape(-1, 3)[rows] += F(0.25)
    for ctx in pair:
        _window(ctx, sc, rows, dense=False, components="r")
        _window(ctx, sc, rows, dense=False, components="tr")
        _window(ctx, sc, np.arange(300, 900), dense=True, components="t")
    check_frame(pair, sc, carried, what="after windows without scale")
    count1, _, launches1 = pair[0].debug_scale_summary_uniform_waves()
    assert count1 == count0
    assert launches1 == launches0, "a window that carries no scale caused a summary launch for the scale part"


@pytest.mark.parametrize("n_views", [2, 4])
def test_several_camera_views(pair, n_views):
    n = 257
    sc = scene(n)
    sc["scale"][3 * 130:3 * 130 + 3] = np.array(ODD, F)  # one mixed wave among the uniform ones
    for ctx in pair:
        upload(ctx, sc)
    carried = Carried(n)
    check_frame(pair, sc, carried, n_views=n_views, what=f"{n_views} views")
    assert_flags(pair[0], n, not_uniform=[2])
    check_frame(pair, sc, carried, n_views=n_views, what=f"{n_views} views, second frame")


def lights_scene():
    sc, first_light, pr = W.frame_scene(257, 300, 100)
    assert first_light == 357 and first_light % 64 != 0
    sc["scale"][:3 * 257] = np.tile(np.array(SCALE, F), 257)  # (the meshes and the lights keep ONE: the waves around the seams are mixed)
    return sc, first_light, pr


@pytest.mark.parametrize("spot", [False, True], ids=["point_lights", "one_spot_light"])
def test_lights_frame_with_the_cluster_walk(pair, spot):
    sc, first_light, pr = lights_scene()
    n, n_lights = sc["n"], 300
    obj_type = spot_dir = sin_cos = None
    if spot:  # (objects are gathered grouped by type: the spot light is the last one)
        obj_type = np.zeros(n_lights, np.uint8)
        obj_type[-1] = 1
        d = np.tile(np.array([0.0, 0.0, 1.0], F), n_lights)
        spot_dir, sin_cos = d, np.tile(np.array([np.sin(0.6), np.cos(0.6)], F), n_lights)
    cam = W.many_cubes_camera(0)
    cfv = api.perspective_clip_from_view(W.CAMERA_FOV, W.CAMERA_ASPECT, W.CAMERA_NEAR)
    fr = api.compute_frustum(cfv, cam, W.CAMERA_FAR)
    view, keep = api.cluster_view_build(cam, cfv, fr, 1920, 1080, (16, 9, 24), 5.0, 1000.0, with_spheres=spot)
    g_exp, vv_exp, _, _ = O.full_frame(sc["translation"], sc["rotation"], sc["scale"], sc["aabb_center"], sc["aabb_half"], sc["flags"], sc["layers"],
                                       np.zeros(n, np.uint8), fr)
    got = []
    for ctx in pair:
        upload(ctx, sc)
        ctx.cluster_upload_objects(pr, obj_type, None, spot_dir, sin_cos)
        ctx.cluster_bind_objects_to_rows(first_light, n_lights)
        ctx.cluster_upload_view(view)
        ctx.propagate_and_cull(fr, flags=B.CULL_END_FRAME | B.CULL_WITH_CLUSTERS)
        g, _ = ctx.download_global_transforms()
        vv, _ = ctx.download_view_visibility()
        assert g.tobytes() == g_exp.tobytes() and vv.tobytes() == vv_exp.tobytes()
        off, idx, counts, far, total = ctx.cluster_download(view.n_clusters)
        got.append((off.tobytes(), idx.tobytes(), counts.tobytes(), np.float32(far).tobytes(), total))
    assert got[0] == got[1], "cluster lists differ from the run without the row summary"
    uniform = np.ones(waves(n), np.uint8)
    uniform[257 >> 6] = 0  # cubes | meshes (the lights' scale is ONE like the meshes')
    assert pair[0].debug_scale_summary_uniform_waves()[1].tobytes() == uniform.tobytes()


def test_changed_rows_frame_after_an_indexed_scale_upload(pair):
    """PROP == 2 reads the column per changed row: the summary is brought up to date all the same, for the all-rows frame behind it."""
    n = 257
    sc = scene(n)
    for ctx in pair:
        upload(ctx, sc)
    carried = Carried(n)
    check_frame(pair, sc, carried, what="uniform")
    rows = np.array([3, 64, 200], np.uint32)
    sc["scale"].reshape(-1, 3)[rows] = np.array(ODD, F)
    fr = frusta_for(1)
    g_exp, vv_exp, _, _ = O.full_frame(sc["translation"], sc["rotation"], sc["scale"], sc["aabb_center"], sc["aabb_half"], sc["flags"], sc["layers"],
                                       carried.vv, fr)
    for ctx in pair:
        ctx.upload_transforms_indexed(rows, *_rows_of(sc, rows))
        ctx.propagate_and_cull(fr, flags=B.CULL_CHANGED_ROWS)
        ctx.visibility_end_frame()
        assert ctx.download_global_transforms()[0].tobytes() == g_exp.tobytes()
        assert ctx.download_view_visibility()[0].tobytes() == vv_exp.tobytes()
    carried.vv = vv_exp
    assert_flags(pair[0], n, not_uniform=[0, 1, 3])
    check_frame(pair, sc, carried, what="all rows again")
