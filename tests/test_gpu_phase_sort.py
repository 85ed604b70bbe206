"""mi_phase_sort (sort_phase_system on the device) against numpy: the expected list from the class mask, the distances in the
library's stated association, and a stable argsort of the mapped u32 key.  The sizes are the seams of the kernels: wave, workgroup
round, the one-workgroup limit PS_ONE_WG_MAX, and several tiles with a ragged last one."""
import ctypes as C

import numpy as np
import pytest

import bevy_amd as B
from bevy_amd import api

pytestmark = pytest.mark.gpu

PS = 8192  # PS_ONE_WG_MAX (kernels.h)
SIZES = [0, 1, 63, 64, 65, 1023, 1025, PS - 1, PS, PS + 1, 2 * PS + 1, 20_000]
F32, F64, U32 = np.float32, np.float64, np.uint32
EVERYTHING = np.tile(np.array([0, 0, 0, 1], F32), 6)  # a frustum that contains every point


def scene(ctx, t, bias=None, keys_descend=False, cls=None):
    """Rows 1, 4, 7, ... carry class bit 1 at translations t[n_items, 3] and are visible; the others carry bit 0; one more row of
    class 1 at the end is hidden, so the list exists (and is empty) at n_items = 0.  -> (rows of the list in Entity order, keys)"""
    n_items = len(t)
    n = 3 * n_items + 4
    rows = np.arange(n_items) * 3 + 1
    g = np.zeros((n, 12), F32)
    g[:, 0] = g[:, 4] = g[:, 8] = 1
    g[rows, 9:12] = t
    mask = np.ones(n, U32)
    mask[rows] = 2
    mask[n - 1] = 2
    flags = np.full(n, B.FLAG_INHERITED_VISIBLE | B.FLAG_NO_FRUSTUM_CULLING, np.uint8)
    flags[n - 1] = 0
    keys = ((n - np.arange(n)) if keys_descend else np.arange(n)).astype(np.uint64) * 7 + 11
    ctx.resize(n)
    ctx.upload_global_transforms(g.reshape(-1))
    ctx.upload_bounds(np.zeros(3 * n, F32), np.zeros(3 * n, F32), flags)
    ctx.upload_visibility_classes(mask if cls is None else cls)
    ctx.upload_entity_keys(keys)
    if bias is not None:
        full = np.zeros(n, F32)
        full[rows] = bias
        ctx.upload_depth_bias(full)
    ctx.cull(EVERYTHING, flags=B.CULL_BEGIN_FRAME | B.CULL_END_FRAME)
    return (rows[::-1] if keys_descend else rows).astype(U32), keys


def check(got, list_rows, keys, dist_of_row):
    """dist_of_row: f32 distance per list entry, in list order"""
    bits = dist_of_row.view(U32)
    key = bits ^ np.where(bits >> 31, U32(0xFFFFFFFF), U32(0x80000000))
    order = np.argsort(key, kind="stable")
    assert np.array_equal(got["rows"], list_rows[order])
    assert np.array_equal(got["entity_keys"], keys[list_rows[order]])
    assert np.array_equal(got["distance"].view(U32), bits[order])


@pytest.mark.parametrize("n", SIZES)
def test_order_all_four_digits(n):
    rng = np.random.default_rng(100 + n)
    bits = (rng.integers(0, 2, (n, 3), dtype=np.uint64) << 31) | (rng.integers(127 - 60, 127 + 61, (n, 3), dtype=np.uint64) << 23) \
        | rng.integers(0, 1 << 23, (n, 3), dtype=np.uint64)
    t = bits.astype(U32).view(F32)
    bias = None
    if n == 2 * PS + 1:  # +-inf through the bias column; everywhere else the column does not exist
        bias = np.zeros(n, F32)
        bias[[5, PS + 9]] = np.inf
        bias[[77, 2 * PS]] = -np.inf
    with B.Context() as ctx:
        rows, keys = scene(ctx, t, bias)
        got = ctx.phase_sort(0, 1, [0, 0, -1, 0])
    x, y, z = t.astype(F64).T
    with np.errstate(invalid="ignore"):
        dist = ((0 * x + -1 * z) + (0 * y + 0 * 1.0)) + (0.0 if bias is None else bias.astype(F64))
    check(got, rows, keys, dist.astype(F32))


# keys_descend: the list comes from the general compaction (segment bases), in key order -- one size per regime
@pytest.mark.parametrize("n,keys_descend", [(n, False) for n in SIZES] + [(65, True), (PS + 1, True)])
def test_ties_keep_entity_order(n, keys_descend):
    rng = np.random.default_rng(200 + n)
    row2 = rng.choice(np.arange(-2, 2.25, 0.25), 4).astype(F32)
    t = rng.integers(-64, 65, (n, 3)).astype(F32)
    bias = rng.choice(np.array([0, 0.25, -0.5], F32), n)
    with B.Context() as ctx:
        rows, keys = scene(ctx, t, bias, keys_descend)
        got = ctx.phase_sort(0, 1, row2)
    r, (x, y, z) = row2.astype(F64), t.astype(F64).T
    dist = ((r[0] * x + r[2] * z) + (r[1] * y + r[3] * 1.0)) + bias.astype(F64)  # every product and sum is exact
    list_t = (rows - 1) // 3  # list entry -> item
    check(got, rows, keys, dist.astype(F32)[list_t])
    assert n < 2000 or len(np.unique(dist)) < n // 4  # most items tie


@pytest.mark.parametrize("n", [1000, 20_000])
def test_general_camera_bits(n):
    rng = np.random.default_rng(300 + n)
    eye, target, up = np.array([30.0, 40.0, -25.0]), np.array([-3.0, 5.0, 8.0]), np.array([0.0, 1.0, 0.0])
    back = (eye - target) / np.linalg.norm(eye - target)  # look_at: the camera looks down its -z
    right = np.cross(up, back) / np.linalg.norm(np.cross(up, back))
    world_from_view = np.eye(4)
    world_from_view[:3, :3] = np.stack([right, np.cross(back, right), back], axis=1)
    world_from_view[:3, 3] = eye
    row2 = np.linalg.inv(world_from_view)[2].astype(F32)
    t = rng.uniform(-100, 100, (n, 3)).astype(F32)
    bias = rng.uniform(-1, 1, n).astype(F32)
    with B.Context() as ctx:
        rows, keys = scene(ctx, t, bias)
        got = ctx.phase_sort(0, 1, row2)
    x, y, z = t.T
    dist = ((row2[0] * x + row2[2] * z) + (row2[1] * y + row2[3] * F32(1))) + bias  # IEEE single, one rounding per operation
    assert dist.dtype == F32
    check(got, rows, keys, dist)
    r = row2.astype(F64)
    exact = r[0] * x.astype(F64) + r[1] * y + r[2] * z + r[3] + bias
    mag = abs(r[0] * x) + abs(r[1] * y) + abs(r[2] * z) + abs(r[3]) + abs(bias.astype(F64))
    order = np.argsort(got["rows"])  # back to list order
    assert np.all(np.abs(got["distance"][order] - exact) <= 4 * 2.0**-24 * mag)


def test_preconditions():
    rng = np.random.default_rng(4)
    n = 300
    t = rng.integers(-64, 65, (n, 3)).astype(F32)
    cnt = C.c_uint32(7)
    with B.Context() as ctx:
        ctx.resize(16)
        with pytest.raises(api.MiError) as e:
            ctx.phase_sort(0, 1, [0, 0, -1, 0])
        assert e.value.code == api.MI_ERR_NOT_READY
        assert ctx._lib.mi_phase_sort_download(ctx._h, None, None, None, 0, C.byref(cnt)) == api.MI_ERR_NOT_READY
        rows, keys = scene(ctx, t)
        with pytest.raises(api.MiError) as e:
            ctx.phase_sort(1, 1, [0, 0, -1, 0])  # the cull had one view
        assert e.value.code == api.MI_ERR_INVALID_ARG
        r2 = np.array([0, 0, -1, 0], F32)
        assert ctx._lib.mi_phase_sort(ctx._h, 0, 1, api._ptr(r2, C.c_float), 1) == api.MI_ERR_INVALID_ARG  # no flag is defined
        assert len(ctx.phase_sort(0, 5, r2)["rows"]) == 0  # a class no row carries
        check(ctx.phase_sort(0, 1, r2), rows, keys, 0 - t[:, 2])
        assert ctx._lib.mi_phase_sort_download(ctx._h, None, None, None, n - 1, C.byref(cnt)) == api.MI_ERR_CAPACITY and cnt.value == n
        # another (view, class) replaces the result: class 0 is every other visible row
        others = np.setdiff1d(np.arange(3 * n + 3, dtype=U32), rows)
        check(ctx.phase_sort(0, 0, r2), others, keys, np.zeros(len(others), F32))
        # a later frame's list is picked up: the odd items leave class 1
        mask = np.ones(3 * n + 4, U32)
        mask[rows[::2]] = 2
        scene(ctx, t, cls=mask)
        check(ctx.phase_sort(0, 1, r2), rows[::2], keys, 0 - t[::2, 2])
