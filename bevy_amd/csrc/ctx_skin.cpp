// ctx_skin.cpp -- skinned meshes: the entry points in front of kernels_skin.hip.  mi_skin_upload checks every index the kernel
// will follow (it tests none of them again) and lays the skins out for it; mi_skin_frame is one launch.
#include "ctx.h"

using namespace mi;
using namespace mi_detail;

extern "C" {

int32_t mi_skin_upload_inverse_bindposes(mi_ctx* ctx, uint32_t first, uint32_t n, const float* mat4) {
    ENTER(ctx);
    if (n == 0) return MI_OK;
    if (!mat4) return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_upload_inverse_bindposes: NULL");
    const uint64_t end = (uint64_t)first + n;
    if (end >= SKIN_GAP_SLOT) return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_upload_inverse_bindposes: matrices [%u,%llu) exceed the pool's index range", first, (unsigned long long)end);
    if (end * 64u > ctx->sk_pool.bytes) {  // grow, keeping what is there; matrices never uploaded are zero
        DevBuf nb;
        int32_t rc = ensure(ctx, nb, (size_t)std::max<uint64_t>(end, (uint64_t)ctx->sk_pool_n * 3u / 2u) * 64u);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemsetAsync(nb.p, 0, nb.bytes, ctx->stream));
        if (ctx->sk_pool.p) {
            HIP_TRY(ctx, hipMemcpyAsync(nb.p, ctx->sk_pool.p, (size_t)ctx->sk_pool_n * 64u, hipMemcpyDeviceToDevice, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipFree(ctx->sk_pool.p));
        }
        ctx->sk_pool = nb;
    }
    ctx->sk_pool_n = std::max<uint32_t>(ctx->sk_pool_n, (uint32_t)end);
    return upload(ctx, (float*)ctx->sk_pool.p + (size_t)first * 16u, mat4, (size_t)n * 64u);
}

int32_t mi_skin_upload(mi_ctx* ctx, uint32_t n_skins, const mi_skin* skins, uint32_t n_slots, const uint32_t* joint_rows, uint32_t n_aabbs,
                       const mi_joint_aabb* aabbs) {
    ENTER(ctx);
    if ((n_skins && !skins) || (n_slots && !joint_rows) || (n_aabbs && !aabbs)) return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_upload: NULL array");
    // ---- validation: nothing of the previous upload is touched before it has passed ----
    std::vector<uint32_t> slot_bind(n_slots, SKIN_GAP_SLOT);
    std::vector<SkinBounded> bounded;
    uint32_t row_end = 0, mesh_lo = 0xFFFFFFFFu, mesh_hi = 0;
    for (uint32_t i = 0; i < n_skins; ++i) {
        const mi_skin& s = skins[i];
        if (s.mesh_row >= ctx->n) return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_upload: skin %u: mesh_row %u >= %u live rows", i, s.mesh_row, ctx->n);
        if ((uint64_t)s.first_joint + s.n_joints > n_slots)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_upload: skin %u: slots [%u,+%u) exceed %u slots", i, s.first_joint, s.n_joints, n_slots);
        if ((uint64_t)s.first_bindpose + s.n_joints > ctx->sk_pool_n)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_upload: skin %u: inverse bindposes [%u,+%u) exceed the %u uploaded", i, s.first_bindpose, s.n_joints, ctx->sk_pool_n);
        if ((uint64_t)s.first_aabb + s.n_aabbs > n_aabbs)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_upload: skin %u: joint AABBs [%u,+%u) exceed %u", i, s.first_aabb, s.n_aabbs, n_aabbs);
        row_end = std::max(row_end, s.mesh_row + 1u);
        for (uint32_t k = 0; k < s.n_joints; ++k) {
            const uint32_t slot = s.first_joint + k, row = joint_rows[slot];
            if (slot_bind[slot] != SKIN_GAP_SLOT) return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_upload: skin %u: slot %u belongs to another skin as well", i, slot);
            slot_bind[slot] = s.first_bindpose + k;
            if (row == MI_SKIN_NO_JOINT) continue;
            if (row >= ctx->n) return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_upload: skin %u: joint %u is row %u >= %u live rows", i, k, row, ctx->n);
            row_end = std::max(row_end, row + 1u);
        }
        for (uint32_t k = 0; k < s.n_aabbs; ++k) {
            const uint32_t j = aabbs[s.first_aabb + k].joint;
            if (j >= s.n_joints) return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_upload: skin %u: joint AABB %u names joint %u of %u", i, k, j, s.n_joints);
            if (joint_rows[s.first_joint + j] == MI_SKIN_NO_JOINT)
                return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_upload: skin %u: joint AABB %u names joint %u, which is MI_SKIN_NO_JOINT", i, k, j);
        }
        if (s.n_aabbs) {
            SkinBounded b{};
            b.mesh_row = s.mesh_row, b.first_joint = s.first_joint, b.first_aabb = s.first_aabb, b.n_aabbs = s.n_aabbs, b.skin = i;
            bounded.push_back(b);
            mesh_lo = std::min(mesh_lo, s.mesh_row);
            mesh_hi = std::max(mesh_hi, s.mesh_row + 1u);
        }
    }
    {
        std::vector<uint32_t> mesh_rows(n_skins);
        for (uint32_t i = 0; i < n_skins; ++i) mesh_rows[i] = skins[i].mesh_row;
        std::sort(mesh_rows.begin(), mesh_rows.end());
        auto dup = std::adjacent_find(mesh_rows.begin(), mesh_rows.end());
        if (dup != mesh_rows.end()) return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_upload: mesh_row %u belongs to two skins", *dup);
    }
    // ---- the device layout ----
    std::vector<uint32_t> soa((size_t)7 * n_aabbs);
    for (uint32_t k = 0; k < n_aabbs; ++k) {
        soa[k] = aabbs[k].joint;
        for (uint32_t e = 0; e < 3; ++e) {
            memcpy(&soa[(size_t)(1 + e) * n_aabbs + k], &aabbs[k].center[e], 4);
            memcpy(&soa[(size_t)(4 + e) * n_aabbs + k], &aabbs[k].half_extents[e], 4);
        }
    }
    ctx->sk_uploaded = false;
    ctx->sk_have_cur = ctx->sk_have_prev = ctx->sk_have_bounds = false;
    ctx->sk_cur = 0;
    int32_t rc;
    if ((rc = ensure(ctx, ctx->sk_joint_rows, (size_t)n_slots * 4))) return rc;
    if ((rc = ensure(ctx, ctx->sk_slot_bind, (size_t)n_slots * 4))) return rc;
    if ((rc = ensure(ctx, ctx->sk_bounded, bounded.size() * sizeof(SkinBounded)))) return rc;
    if ((rc = ensure(ctx, ctx->sk_aabbs, soa.size() * 4))) return rc;
    if ((rc = ensure(ctx, ctx->sk_bounds, (size_t)n_skins * 24))) return rc;
    for (DevBuf& m : ctx->sk_mats) {  // (zeroed: a slot no skin owns is never written)
        if ((rc = ensure(ctx, m, (size_t)n_slots * 64))) return rc;
        HIP_TRY(ctx, hipMemsetAsync(m.p, 0, m.bytes, ctx->stream));
    }
    if ((rc = upload(ctx, ctx->sk_joint_rows.p, joint_rows, (size_t)n_slots * 4))) return rc;
    if ((rc = upload(ctx, ctx->sk_slot_bind.p, slot_bind.data(), (size_t)n_slots * 4))) return rc;
    if ((rc = upload(ctx, ctx->sk_bounded.p, bounded.data(), bounded.size() * sizeof(SkinBounded)))) return rc;
    if ((rc = upload(ctx, ctx->sk_aabbs.p, soa.data(), soa.size() * 4))) return rc;
    ctx->sk_skins.assign(skins, skins + n_skins);
    ctx->sk_n_slots = n_slots;
    ctx->sk_n_bounded = (uint32_t)bounded.size();
    ctx->sk_n_aabbs = n_aabbs;
    ctx->sk_row_end = row_end;
    ctx->sk_mesh_lo = bounded.empty() ? 0u : mesh_lo;
    ctx->sk_mesh_hi = mesh_hi;
    ctx->sk_uploaded = true;
    return MI_OK;
}

int32_t mi_skin_frame(mi_ctx* ctx, uint32_t flags) {
    ENTER(ctx);
    const uint32_t known = MI_SKIN_MATRICES | MI_SKIN_BOUNDS | MI_SKIN_KEEP_PREVIOUS;
    if ((flags & ~known) || !(flags & (MI_SKIN_MATRICES | MI_SKIN_BOUNDS))) return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_frame: flags 0x%x", flags);
    if ((flags & MI_SKIN_KEEP_PREVIOUS) && !(flags & MI_SKIN_MATRICES)) return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_frame: MI_SKIN_KEEP_PREVIOUS without MI_SKIN_MATRICES");
    if (!ctx->sk_uploaded) return fail(ctx, MI_ERR_NOT_READY, "mi_skin_frame before mi_skin_upload");
    if (ctx->sk_row_end > ctx->n)
        return fail(ctx, MI_ERR_NOT_READY, "mi_skin_frame: the skins reference row %u, the context has %u rows (upload the skins again)", ctx->sk_row_end - 1u, ctx->n);
    if (flags & MI_SKIN_MATRICES) {
        if (flags & MI_SKIN_KEEP_PREVIOUS) {
            ctx->sk_have_prev = ctx->sk_have_cur;
            ctx->sk_cur ^= 1u;
        }
        ctx->sk_have_cur = true;
    }
    SkinArgs a{};
    uint32_t n_bounds_wgs = 0;
    skin_grid(ctx->sk_n_slots, ctx->sk_n_bounded, (flags & MI_SKIN_MATRICES) != 0, (flags & MI_SKIN_BOUNDS) != 0, &a.n_mat_wgs, &n_bounds_wgs);
    if (flags & MI_SKIN_BOUNDS) {
        ctx->sk_have_bounds = true;
        if (n_bounds_wgs) {
            // The Aabb columns of the mesh rows are about to change under whatever was derived from them -- as in mi_upload_bounds:
            // the world spheres, the row summary's Aabb part (the smallest covering range of rows) and, through row_summary_touch,
            // the static cull order; and an assignment on the cluster stream may still be reading the columns.
            int32_t rc = cluster_join(ctx);
            if (rc) return rc;
            ctx->cl_inputs_dirty = true;
            ctx->sph_state = mi_ctx::SPH_INVALID;
            row_summary_touch(ctx, ROWSUM_PART_AABB, ctx->sk_mesh_lo, ctx->sk_mesh_hi - ctx->sk_mesh_lo);
        }
    }
    a.n_slots = ctx->sk_n_slots;
    a.n_bounded = ctx->sk_n_bounded;
    a.n_aabbs = ctx->sk_n_aabbs;
    a.joint_rows = (const uint32_t*)ctx->sk_joint_rows.p;
    a.slot_bindpose = (const uint32_t*)ctx->sk_slot_bind.p;
    a.bindposes = (const float*)ctx->sk_pool.p;
    a.global = ctx->g;
    a.matrices = (float*)ctx->sk_mats[ctx->sk_cur].p;
    a.bounded = (const SkinBounded*)ctx->sk_bounded.p;
    a.aabbs = (const uint32_t*)ctx->sk_aabbs.p;
    a.aabb_center = ctx->c;
    a.aabb_half = ctx->h;
    a.skin_bounds = (float*)ctx->sk_bounds.p;
    HIP_TRY(ctx, launch_skin_frame(a, n_bounds_wgs, ctx->stream));
    return MI_OK;
}

int32_t mi_skin_download_matrices(mi_ctx* ctx, uint32_t which, uint32_t first_slot, uint32_t n, float* out16) {
    ENTER(ctx);
    if (which > 1u) return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_download_matrices: which = %u", which);
    if (!ctx->sk_uploaded || !(which ? ctx->sk_have_prev : ctx->sk_have_cur))
        return fail(ctx, MI_ERR_NOT_READY, "mi_skin_download_matrices: no %s matrices yet", which ? "previous" : "current");
    if ((uint64_t)first_slot + n > ctx->sk_n_slots)
        return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_download_matrices: slots [%u,+%u) exceed %u", first_slot, n, ctx->sk_n_slots);
    if (n == 0) return MI_OK;
    if (!out16) return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_download_matrices: NULL");
    return download(ctx, out16, (const float*)ctx->sk_mats[ctx->sk_cur ^ which].p + (size_t)first_slot * 16u, (size_t)n * 64u);
}

int32_t mi_skin_download_bounds(mi_ctx* ctx, uint32_t first_skin, uint32_t n, float* center3, float* half3) {
    ENTER(ctx);
    if (!ctx->sk_uploaded || !ctx->sk_have_bounds) return fail(ctx, MI_ERR_NOT_READY, "mi_skin_download_bounds before a mi_skin_frame with MI_SKIN_BOUNDS");
    if (ctx->sk_row_end > ctx->n) return fail(ctx, MI_ERR_NOT_READY, "mi_skin_download_bounds: the skins reference row %u, the context has %u rows", ctx->sk_row_end - 1u, ctx->n);
    if ((uint64_t)first_skin + n > ctx->sk_skins.size())
        return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_download_bounds: skins [%u,+%u) exceed %zu", first_skin, n, ctx->sk_skins.size());
    if (n == 0) return MI_OK;
    if (!center3 || !half3) return fail(ctx, MI_ERR_INVALID_ARG, "mi_skin_download_bounds: NULL");
    std::vector<float> both((size_t)n * 6);
    int32_t rc = download(ctx, both.data(), (const float*)ctx->sk_bounds.p + (size_t)first_skin * 6u, both.size() * 4);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        const mi_skin& s = ctx->sk_skins[first_skin + i];
        if (s.n_aabbs) {
            memcpy(center3 + 3 * (size_t)i, &both[6 * (size_t)i], 12);
            memcpy(half3 + 3 * (size_t)i, &both[6 * (size_t)i + 3], 12);
        } else {  // no joint AABBs: the frame left the row's Aabb alone, and that is what the skin reports
            if ((rc = download(ctx, center3 + 3 * (size_t)i, ctx->c + 3 * (size_t)s.mesh_row, 12))) return rc;
            if ((rc = download(ctx, half3 + 3 * (size_t)i, ctx->h + 3 * (size_t)s.mesh_row, 12))) return rc;
        }
    }
    return MI_OK;
}

}  // extern "C"
