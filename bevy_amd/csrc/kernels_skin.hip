// kernels_skin.hip -- skinned meshes behind the propagate: the joint matrices extract_skins computes per joint and the Aabb
// update_skinned_mesh_bounds refits per mesh, in ONE launch whose workgroups take one of two roles by blockIdx (kernels.h, SkinArgs).
//
//   matrix workgroups [0, n_mat_wgs)      a QUAD of lanes owns a slot, a lane one column of its matrix: 16 slots per wave, 64 per
//     workgroup.  Lane c fetches column c of the slot's inverse bindpose (16 bytes; a wave whose slots follow each other in the
//     pool reads 1 KB contiguously) and lanes 0..2 one 16-byte third each of the joint's 48-byte GlobalTransform row; the twelve
//     floats reach all four lanes as DPP quad_perm broadcasts (register moves: no LDS, and no lane fetches the row three times).
//     The lane's column  ((x_axis b.x + y_axis b.y) + z_axis b.z) + w_axis b.w  leaves as one nontemporal 16-byte store: nobody
//     on this device reads it back before the render world does, and a wave writes 1 KB contiguously.
//   bounds workgroups [n_mat_wgs, ...)    a WAVE owns a skin with joint AABBs.  Its descriptor and the mesh's GlobalTransform are
//     wave-uniform (scalar) loads, E = inverse(mesh) is computed once; lane l takes the AABBs l, l + 64, ..., gathers each one's
//     joint row and keeps a private min / max corner (from +-inf).  The six values are folded across the wave by DPP row shifts
//     and row broadcasts (no LDS, no atomics); lane 0 writes the Aabb columns of the mesh's row and the per-skin array.
// Arithmetic: glam_math.h throughout (every operation rounded on its own; -ffp-contract=off).
#include "glam_math.h"
#include "kernels.h"

namespace mi {

namespace {
constexpr uint32_t SKIN_THREADS = 256;

template <int K>
__device__ __forceinline__ float sk_quad_bcast(float v) {  // lane K of every quad -> its four lanes (v_mov_b32 quad_perm)
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), K * 0x55, 0xF, 0xF, true));
}

// One step of the wave fold: v = op(v, v of the lane the DPP control names).  Lanes the control gives no source (the first lanes
// of a row under row_shr, the rows masked out of a broadcast) read `identity`, which leaves their value as it is.
template <bool MIN, int CTRL, int ROW_MASK>
__device__ __forceinline__ float sk_fold_step(float v, float identity) {
    const float o = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(identity), __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
    return MIN ? lane_min(v, o) : lane_max(v, o);
}
// min / max over the 64 lanes, uniform result: row_shr 1, 2, 4, 8 leave each row's fold in its lane 15, row_bcast15 carries rows
// 0 and 2 into rows 1 and 3, row_bcast31 the lower half into the upper: lane 63 holds the wave's.
template <bool MIN>
__device__ __forceinline__ float sk_wave_fold(float v) {
    const float id = MIN ? __builtin_inff() : -__builtin_inff();
    v = sk_fold_step<MIN, 0x111, 0xF>(v, id);
    v = sk_fold_step<MIN, 0x112, 0xF>(v, id);
    v = sk_fold_step<MIN, 0x114, 0xF>(v, id);
    v = sk_fold_step<MIN, 0x118, 0xF>(v, id);
    v = sk_fold_step<MIN, 0x142, 0xA>(v, id);
    v = sk_fold_step<MIN, 0x143, 0xC>(v, id);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

__device__ __forceinline__ void skin_matrices(const SkinArgs& a, uint32_t gid) {
    const uint32_t slot = gid >> 2, col = gid & 3u;
    uint32_t bind = SKIN_GAP_SLOT, row = SKIN_NO_JOINT;
    if (slot < a.n_slots) {
        bind = a.slot_bindpose[slot];
        row = a.joint_rows[slot];
    }
    // (whole quads take these branches together: the four lanes of a quad share the slot)
    const bool live = bind != SKIN_GAP_SLOT, jointed = live && row != SKIN_NO_JOINT;
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f), gp = b;
    if (live) b = reinterpret_cast<const float4*>(a.bindposes)[(size_t)bind * 4u + col];
    if (jointed && col < 3u) gp = reinterpret_cast<const float4*>(a.global)[(size_t)row * 3u + col];
    // every lane of the wave runs the broadcasts: lane 0 of the quad holds floats 0..3 of the row, lane 1 4..7, lane 2 8..11
    Affine g;
    g.m.x_axis = V3{sk_quad_bcast<0>(gp.x), sk_quad_bcast<0>(gp.y), sk_quad_bcast<0>(gp.z)};
    g.m.y_axis = V3{sk_quad_bcast<0>(gp.w), sk_quad_bcast<1>(gp.x), sk_quad_bcast<1>(gp.y)};
    g.m.z_axis = V3{sk_quad_bcast<1>(gp.z), sk_quad_bcast<1>(gp.w), sk_quad_bcast<2>(gp.x)};
    g.t = V3{sk_quad_bcast<2>(gp.y), sk_quad_bcast<2>(gp.z), sk_quad_bcast<2>(gp.w)};
    const V4 o = mul(m4_from_affine(g), V4{b.x, b.y, b.z, b.w});  // (the w row in full: 0 b.x + 0 b.y + 0 b.z + 1 b.w)
    typedef float v4f_t __attribute__((ext_vector_type(4)));
    // a slot whose joint is MI_SKIN_NO_JOINT gets its bindpose, bit for bit
    const v4f_t out = jointed ? v4f_t{o.x, o.y, o.z, o.w} : v4f_t{b.x, b.y, b.z, b.w};
    if (live) __builtin_nontemporal_store(out, reinterpret_cast<v4f_t*>(a.matrices) + ((size_t)slot * 4u + col));
}

__device__ __forceinline__ void skin_bounds(const SkinArgs& a, uint32_t wave, uint32_t lane) {
    // wave-uniform: the descriptor and the mesh's row go through scalar loads
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave);
    const SkinBounded d = a.bounded[w];
    const uint32_t mesh_row = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.mesh_row);
    const Affine e = inverse(load_affine(a.global + (size_t)mesh_row * 12u));
    const float inf = __builtin_inff();
    V3 lo = V3{inf, inf, inf}, hi = V3{-inf, -inf, -inf};
    const size_t col = a.n_aabbs;  // the AABBs are seven columns of n_aabbs words: joint, centre x y z, half extents x y z
    for (uint32_t k = lane; k < d.n_aabbs; k += 64u) {
        const size_t at = (size_t)d.first_aabb + k;
        const uint32_t row = a.joint_rows[d.first_joint + a.aabbs[at]];  // (the upload refused a MI_SKIN_NO_JOINT here)
        const float* f = reinterpret_cast<const float*>(a.aabbs) + at;
        const V3 c = V3{f[col], f[2 * col], f[3 * col]}, h = V3{f[4 * col], f[5 * col], f[6 * col]};
        const float4* gr = reinterpret_cast<const float4*>(a.global) + (size_t)row * 3u;
        const float4 g0 = gr[0], g1 = gr[1], g2 = gr[2];
        Affine g;
        g.m.x_axis = V3{g0.x, g0.y, g0.z};
        g.m.y_axis = V3{g0.w, g1.x, g1.y};
        g.m.z_axis = V3{g1.z, g1.w, g2.x};
        g.t = V3{g2.y, g2.z, g2.w};
        const Affine m = mul(e, g);  // mesh_from_joint
        const V3 cc = transform_point(m, c);
        const V3 hh = mul(M3{abs3(m.m.x_axis), abs3(m.m.y_axis), abs3(m.m.z_axis)}, h);
        lo = min3(lo, cc - hh);
        hi = max3(hi, cc + hh);
    }
    lo = V3{sk_wave_fold<true>(lo.x), sk_wave_fold<true>(lo.y), sk_wave_fold<true>(lo.z)};
    hi = V3{sk_wave_fold<false>(hi.x), sk_wave_fold<false>(hi.y), sk_wave_fold<false>(hi.z)};
    if (lane == 0u) {  // Aabb::from_min_max
        const V3 center = (hi + lo) * 0.5f, half = (hi - lo) * 0.5f;
        float* c = a.aabb_center + (size_t)mesh_row * 3u;
        float* h = a.aabb_half + (size_t)mesh_row * 3u;
        float* o = a.skin_bounds + (size_t)d.skin * 6u;
        c[0] = center.x, c[1] = center.y, c[2] = center.z;
        h[0] = half.x, h[1] = half.y, h[2] = half.z;
        o[0] = center.x, o[1] = center.y, o[2] = center.z;
        o[3] = half.x, o[4] = half.y, o[5] = half.z;
    }
}

__global__ __launch_bounds__(SKIN_THREADS) void k_skin_frame(SkinArgs a) {
    if (blockIdx.x < a.n_mat_wgs) {
        skin_matrices(a, blockIdx.x * SKIN_THREADS + threadIdx.x);
        return;
    }
    const uint32_t wave = (blockIdx.x - a.n_mat_wgs) * (SKIN_THREADS / 64u) + (threadIdx.x >> 6);
    if (wave < a.n_bounded) skin_bounds(a, wave, threadIdx.x & 63u);
}
}  // namespace

void skin_grid(uint32_t n_slots, uint32_t n_bounded, bool matrices, bool bounds, uint32_t* n_mat_wgs, uint32_t* n_bounds_wgs) {
    *n_mat_wgs = matrices ? (uint32_t)((4ull * n_slots + SKIN_THREADS - 1u) / SKIN_THREADS) : 0u;
    *n_bounds_wgs = bounds ? (n_bounded + 3u) / 4u : 0u;
}

hipError_t launch_skin_frame(const SkinArgs& a, uint32_t n_bounds_wgs, hipStream_t stream) {
    const uint32_t grid = a.n_mat_wgs + n_bounds_wgs;
    if (grid == 0) return hipSuccess;
    MI_LAUNCH(k_skin_frame, dim3(grid), dim3(SKIN_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace mi
