"""mi_skin_frame (joint matrices and refitted Aabbs on the device) against numpy, at the kernel's seams: a quad per slot, 16 slots per
wave, 64 per workgroup; a wave per bounded skin, 64 joint AABBs per round, 4 skins per workgroup.  Two input families:
  exact   90-degree rotations x power-of-two scales, small integers elsewhere: every intermediate is representable, the device must
          equal an f64 evaluation exactly;
  random  the device must equal the f32 restatement below (the association the header states) bit for bit."""
import ctypes as C

import numpy as np
import pytest

import bevy_amd as B
from bevy_amd import api

pytestmark = pytest.mark.gpu

F32, F64, U32 = np.float32, np.float64, np.uint32
NOJ = B.SKIN_NO_JOINT
WHOLE = B.CULL_BEGIN_FRAME | B.CULL_END_FRAME


def affines(rng, n, family):
    """[n, 12] GlobalTransforms: x_axis, y_axis, z_axis, translation"""
    if family == "random":
        return rng.normal(0, 2, (n, 12)).astype(F32)
    g = np.zeros((n, 4, 3), F32)
    for i in range(n):
        g[i, np.arange(3), rng.permutation(3)] = rng.choice([-1, 1], 3) * 2.0 ** rng.integers(-1, 2, 3)
    g[:, 3] = rng.integers(-8, 9, (n, 3))
    return g.reshape(n, 12)


def values(rng, shape, family):
    return (rng.integers(-4, 5, shape) if family == "exact" else rng.normal(0, 2, shape)).astype(F32)


def m3v(m, v):
    """Mat3A * Vec3A: m[..., column, row], ((X v.x) + Y v.y) + Z v.z"""
    return (m[..., 0, :] * v[..., 0:1] + m[..., 1, :] * v[..., 1:2]) + m[..., 2, :] * v[..., 2:3]


def mat_ref(g, b, dt):
    """Mat4::from(G) * B per slot in dtype dt: column c = ((x_axis b.x + y_axis b.y) + z_axis b.z) + w_axis b.w, the w row in full"""
    b = b.astype(dt).reshape(-1, 4, 4)
    axes = np.zeros((len(g), 4, 4), dt)
    axes[:, :, :3] = g.astype(dt).reshape(-1, 4, 3)
    axes[:, 3, 3] = 1
    out = np.empty_like(b)
    for c in range(4):
        out[:, c] = ((axes[:, 0] * b[:, c, 0:1] + axes[:, 1] * b[:, c, 1:2]) + axes[:, 2] * b[:, c, 2:3]) + axes[:, 3] * b[:, c, 3:4]
    return out.reshape(-1, 16)


def bounds_ref(g, mesh_row, rows, c, h, dt):
    """The refit of one skin: rows[k] = the joint row of AABB k.  glam's Affine3A::inverse, Affine * Affine, Aabb::from_min_max."""
    x, y, z, t = g[mesh_row].astype(dt).reshape(4, 3)
    cross = lambda a, b: np.array([a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]], dt)
    t2 = cross(x, y)
    inv = dt(1) / ((z[0] * t2[0] + z[1] * t2[1]) + z[2] * t2[2])
    em = np.stack([cross(y, z) * inv, cross(z, x) * inv, t2 * inv]).T.copy()  # [column, row]
    et = -m3v(em, t)
    gj = g[rows].astype(dt).reshape(-1, 4, 3)
    am = np.stack([m3v(em, gj[:, i]) for i in range(3)], axis=1)
    cc = m3v(am, c.astype(dt)) + (m3v(em, gj[:, 3]) + et)
    hh = m3v(np.abs(am), h.astype(dt))
    lo, hi = (cc - hh).min(0), (cc + hh).max(0)
    return (hi + lo) * dt(0.5), (hi - lo) * dt(0.5)


def same(got, want, family):
    if family == "exact":
        return np.array_equal(got.astype(F64), want)
    return np.array_equal(got.view(U32), want.view(U32))


def slot_layout(n_slots, extras):
    """Skins of 1, 3, 24, 68, 1, ... slots until n_slots are used up; extras: slot 1 is a gap, skin 1 shares the head of skin 2's
    bindposes.  -> skins [k, 6] (mesh_row = n_slots + index), the bindpose index of every slot (-1: gap)"""
    skins, bind, at = [], np.full(n_slots, -1), 0
    while at < n_slots:
        k = min([1, 3, 24, 68][len(skins) % 4], n_slots - at)
        skins.append([n_slots + len(skins), at, k, at, 0, 0])
        at += k + (1 if extras and len(skins) == 1 else 0)
    if extras:
        skins[1][3] = skins[2][3]
    for s in skins:
        bind[s[1]:s[1] + s[2]] = s[3] + np.arange(s[2])
    return np.array(skins, U32), bind


@pytest.mark.parametrize("family,n_slots", [("exact", n) for n in (1, 15, 16, 17, 63, 64, 65, 200)] + [("random", 17), ("random", 200)])
def test_matrices(family, n_slots):
    rng = np.random.default_rng(n_slots)
    extras = n_slots >= 17
    skins, bind = slot_layout(n_slots, extras)
    n = n_slots + len(skins)
    g, pool = affines(rng, n, family), values(rng, (n_slots, 16), family)
    rows = rng.permutation(n_slots).astype(U32)
    if extras:
        rows[n_slots - 1] = NOJ
    hip = C.CDLL("libamdhip64.so")
    fill = np.full((n_slots, 16), 7.0, F32)
    with B.Context() as ctx:
        ctx.resize(n)
        ctx.upload_global_transforms(g.reshape(-1))
        ctx.upload_inverse_bindposes(pool)
        ctx.upload_skins(skins, rows)
        ctx.synchronize()
        p, nbytes = ctx.device_buffer(api.BUF_JOINT_MATRICES)
        assert nbytes == fill.nbytes and hip.hipMemcpy(C.c_void_p(p), C.c_void_p(fill.ctypes.data), C.c_size_t(nbytes), 1) == 0
        ctx.skin_frame(bounds=False)
        got = ctx.download_joint_matrices()
    live = bind >= 0
    assert extras == (not live.all()) and np.array_equal(got[~live], fill[~live])  # the gap slot is untouched
    jointed = live & (rows != NOJ)
    assert np.array_equal(got[live & ~jointed].view(U32), pool[bind[live & ~jointed]].view(U32))  # no joint: the bindpose's bits
    gj, bj = g[rows[jointed]], pool[bind[jointed]]
    assert same(got[jointed], mat_ref(gj, bj, F64 if family == "exact" else F32), family)
    if family == "random":  # four-term product sums: gamma_4 x sum |a_i b_i| (a layout mistake both restatements might share)
        u = 2.0 ** -24
        assert np.all(np.abs(got[jointed] - mat_ref(gj, bj, F64)) <= 4 * u / (1 - 4 * u) * mat_ref(np.abs(gj), np.abs(bj), F64))


@pytest.mark.parametrize("family", ["exact", "random"])
@pytest.mark.parametrize("n_skins,per_skin", [(1, 1), (1, 63), (1, 64), (1, 65), (4, 130), (5, 7)])
def test_bounds(family, n_skins, per_skin):
    rng = np.random.default_rng(1000 * n_skins + per_skin)
    n_slots = n_skins * per_skin
    n = n_slots + n_skins
    g = affines(rng, n, family)
    rows = rng.permutation(n).astype(U32)  # slots first, then the meshes
    a_joint = np.concatenate([rng.permutation(per_skin) for _ in range(n_skins)]).astype(U32)  # every joint once, shuffled
    a_c, a_h = values(rng, (n_slots, 3), family), np.abs(values(rng, (n_slots, 3), family))
    skins = np.array([[rows[n_slots + i], i * per_skin, per_skin, 0, i * per_skin, per_skin] for i in range(n_skins)], U32)
    if n_skins == 5:
        skins[2, 5] = 0  # no DynamicSkinnedMeshBounds
    c0, h0 = np.tile(np.array([1, 2, 3], F32), n), np.tile(np.array([4, 5, 6], F32), n)
    with B.Context() as ctx:
        ctx.resize(n)
        ctx.upload_global_transforms(g.reshape(-1))
        ctx.upload_bounds(c0, h0)
        ctx.upload_inverse_bindposes(np.zeros((per_skin, 16), F32))
        ctx.upload_skins(skins, rows[:n_slots], a_joint, a_c, a_h)
        ctx.skin_frame(matrices=False)
        got_c, got_h = ctx.download_skin_bounds()
    dt = F64 if family == "exact" else F32
    for i, s in enumerate(skins):
        if s[5] == 0:
            assert np.array_equal(got_c[i], c0[:3]) and np.array_equal(got_h[i], h0[:3])
            continue
        k = slice(s[4], s[4] + s[5])
        want_c, want_h = bounds_ref(g, s[0], rows[s[1] + a_joint[k]], a_c[k], a_h[k], dt)
        assert same(got_c[i], want_c, family) and same(got_h[i], want_h, family), (i, got_c[i], want_c, got_h[i], want_h)


@pytest.mark.parametrize("sphere_path", [0, 2])
def test_bounds_reach_the_cull(sphere_path):
    """130 rows with one bind-pose box (their waves are summary-uniform), a frustum |x| < 10.  Row 5 stands inside, but its joint
    carries its box to x = 50; row 100 stands at x = 100, its joint carries the box back to the origin."""
    n, a, b = 130, 5, 100
    g = np.zeros((n, 12), F32)
    g[:, 0] = g[:, 4] = g[:, 8] = 1
    g[b, 9], g[128, 9] = 100, 50  # rows 128 / 129: the joints of a / b
    frustum = np.tile(np.array([0, 0, 0, 1], F32), 6).reshape(6, 4)
    frustum[0], frustum[1] = [1, 0, 0, 10], [-1, 0, 0, 10]
    skins = np.array([[a, 0, 1, 0, 0, 1], [b, 1, 1, 0, 1, 1]], U32)
    with B.Context() as ctx:
        ctx.debug_set_sphere_path(sphere_path)
        ctx.resize(n)
        ctx.upload_global_transforms(g.reshape(-1))
        ctx.upload_bounds(np.zeros(3 * n, F32), np.ones(3 * n, F32))
        ctx.upload_inverse_bindposes(np.zeros((1, 16), F32))
        ctx.upload_skins(skins, np.array([128, 129], U32), np.zeros(2, U32), np.zeros((2, 3), F32), np.ones((2, 3), F32))
        for _ in range(2):  # (the second quiet frame is the one that takes the sphere column by default)
            ctx.cull(frustum.reshape(-1), flags=WHOLE)
            vis = ctx.download_visibility()
            assert vis[a] == 1 and vis[b] == 0 and vis.sum() == n - 2
        ctx.skin_frame(matrices=False)
        for _ in range(2):
            ctx.cull(frustum.reshape(-1), flags=WHOLE)
            vis = ctx.download_visibility()
            assert vis[a] == 0 and vis[b] == 1 and vis.sum() == n - 2
        c, h = ctx.download_skin_bounds()
    assert np.array_equal(c, [[50, 0, 0], [-100, 0, 0]]) and np.array_equal(h, np.ones((2, 3)))


@pytest.mark.parametrize("n_slots", [5, 70])
def test_previous_matrices(n_slots):
    rng = np.random.default_rng(n_slots)
    g1, g2, pool = affines(rng, n_slots + 1, "random"), affines(rng, n_slots + 1, "random"), values(rng, (n_slots, 16), "random")
    with B.Context() as ctx:
        ctx.resize(n_slots + 1)
        ctx.upload_inverse_bindposes(pool)
        ctx.upload_skins([[n_slots, 0, n_slots, 0, 0, 0]], np.arange(n_slots))
        ctx.upload_global_transforms(g1.reshape(-1))
        ctx.skin_frame(bounds=False, keep_previous=True)
        first = ctx.download_joint_matrices()
        with pytest.raises(api.MiError) as e:
            ctx.download_joint_matrices(which=1)  # nothing came before the first frame
        assert e.value.code == api.MI_ERR_NOT_READY
        ctx.upload_global_transforms(g2.reshape(-1))
        ctx.skin_frame(bounds=False, keep_previous=True)
        assert np.array_equal(ctx.download_joint_matrices(which=1).view(U32), first.view(U32))
        assert np.array_equal(ctx.download_joint_matrices().view(U32), mat_ref(g2[:n_slots], pool, F32).view(U32))
    assert np.array_equal(first.view(U32), mat_ref(g1[:n_slots], pool, F32).view(U32)) and not np.array_equal(g1, g2)


BAD = {  # name -> (skins, joint_rows, joint of the one AABB), in a context of 8 rows and a pool of 4 matrices
    "overlapping slots": ([[6, 0, 3, 0, 0, 0], [7, 2, 2, 0, 0, 0]], [0, 1, 2, 3], 0),
    "duplicate mesh_row": ([[6, 0, 2, 0, 0, 0], [6, 2, 2, 0, 0, 0]], [0, 1, 2, 3], 0),
    "aabb joint": ([[6, 0, 2, 0, 0, 1], [7, 2, 2, 0, 0, 0]], [0, 1, 2, 3], 2),
    "row beyond n": ([[6, 0, 2, 0, 0, 0], [7, 2, 2, 0, 0, 0]], [0, 1, 2, 8], 0),
}


@pytest.mark.parametrize("case", list(BAD) + ["frame before upload", "frame after shrink"])
def test_preconditions(case):
    rng = np.random.default_rng(6)
    g, pool = affines(rng, 8, "exact"), values(rng, (4, 16), "exact")
    good = ([[6, 0, 2, 0, 0, 1], [7, 2, 2, 0, 0, 0]], np.array([0, 1, 2, NOJ], U32))
    box = (np.zeros((1, 3), F32), np.ones((1, 3), F32))
    with B.Context() as ctx:
        ctx.resize(8)
        ctx.upload_global_transforms(g.reshape(-1))
        ctx.upload_inverse_bindposes(pool)
        with pytest.raises(api.MiError) as e:
            if case in BAD:
                ctx.upload_skins(BAD[case][0], BAD[case][1], np.array([BAD[case][2]], U32), *box)
            else:
                if case == "frame after shrink":
                    ctx.upload_skins(*good, np.zeros(1, U32), *box)
                    ctx.resize(7)
                ctx.skin_frame()
        assert e.value.code == (api.MI_ERR_INVALID_ARG if case in BAD else api.MI_ERR_NOT_READY)
        # the context is usable: a good upload (again) and a frame
        ctx.resize(8)
        ctx.upload_global_transforms(g.reshape(-1))
        ctx.upload_skins(*good, np.zeros(1, U32), *box)
        ctx.skin_frame()
        got = ctx.download_joint_matrices()
        c, h = ctx.download_skin_bounds(0, 1)
    assert np.array_equal(got[:3].astype(F64), mat_ref(g[:3], pool[[0, 1, 0]], F64)) and np.array_equal(got[3], pool[1])
    want_c, want_h = bounds_ref(g, 6, np.array([0]), *box, F64)
    assert np.array_equal(c[0].astype(F64), want_c) and np.array_equal(h[0].astype(F64), want_h)
