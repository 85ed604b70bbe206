// ctx_phase_sort.cpp -- sort_phase_system for one (view, class): the entry points in front of kernels_phase_sort.hip.
#include "ctx.h"

using namespace mi;
using namespace mi_detail;

extern "C" {

int32_t mi_upload_depth_bias(mi_ctx* ctx, uint32_t first_row, uint32_t n, const float* depth_bias) {
    ENTER(ctx);
    if (!depth_bias) return fail(ctx, MI_ERR_INVALID_ARG, "mi_upload_depth_bias: NULL");
    int32_t rc = check_rows(ctx, first_row, n, "mi_upload_depth_bias");
    if (rc) return rc;
    if (!ctx->depth_bias && (rc = grow_column(ctx, ctx->depth_bias, 1, 0, ctx->cap, 0))) return rc;  // the column appears with its first use
    if (n == 0) return MI_OK;
    return upload(ctx, ctx->depth_bias + first_row, depth_bias, (size_t)n * 4);
}

int32_t mi_phase_sort(mi_ctx* ctx, uint32_t view, uint32_t class_bit, const float view_from_world_row2[4], uint32_t flags) {
    ENTER(ctx);
    if (!ctx->culled) return fail(ctx, MI_ERR_NOT_READY, "mi_phase_sort before mi_cull");
    if (flags) return fail(ctx, MI_ERR_INVALID_ARG, "mi_phase_sort: unknown flags 0x%x", flags);
    if (!view_from_world_row2) return fail(ctx, MI_ERR_INVALID_ARG, "mi_phase_sort: NULL view_from_world_row2");
    {
        int32_t rcj = compaction_join(ctx);  // asynchronous compaction: the list this sort reads must be complete
        if (rcj) return rcj;
    }
    if (view >= ctx->compact_views) return fail(ctx, MI_ERR_INVALID_ARG, "mi_phase_sort: view %u of %u", view, ctx->compact_views);
    uint32_t slot = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < ctx->compact_classes; ++k)
        if (ctx->class_bits[k] == class_bit) slot = k;
    if (slot == 0xFFFFFFFFu || ctx->n == 0) {  // no row carries this class: VisibleEntities::get() is empty -> so is the phase
        ctx->ps_state = mi_ctx::PS_EMPTY;
        return MI_OK;
    }
    int32_t rc;
    if (!ctx->ps_lds_set) {
        HIP_TRY(ctx, set_phase_sort_lds_limit());
        ctx->ps_lds_set = true;
    }
    PhaseSortArgs a{};
    a.n = ctx->n;
    if ((rc = ensure(ctx, ctx->ps_rows, (size_t)ctx->n * 4))) return rc;
    if ((rc = ensure(ctx, ctx->ps_keys, (size_t)ctx->n * 8))) return rc;
    if ((rc = ensure(ctx, ctx->ps_dist, (size_t)ctx->n * 4))) return rc;
    if ((rc = ensure(ctx, ctx->ps_count, 64))) return rc;
    if (ctx->n > PS_ONE_WG_MAX) {
        const size_t tiles = ((size_t)ctx->n + PS_ONE_WG_MAX - 1u) / PS_ONE_WG_MAX;
        for (int k = 0; k < 2; ++k) {
            if ((rc = ensure(ctx, ctx->ps_pairs[k], tiles * PS_ONE_WG_MAX * 8))) return rc;
            a.pairs[k] = (uint64_t*)ctx->ps_pairs[k].p;
        }
        if ((rc = ensure(ctx, ctx->ps_table, tiles * PS_DIGITS * 4))) return rc;
        a.table = (uint32_t*)ctx->ps_table.p;
    }
    const uint32_t seg = view * ctx->compact_classes + slot;
    a.list_count = (const uint32_t*)ctx->fb[ctx->cur].seg_totals.p + seg;
    if (ctx->compact_fast) {
        a.list = (const uint32_t*)ctx->fb[ctx->cur].out_rows.p + (size_t)seg * ctx->seg_stride;
        a.list_base = nullptr;
    } else {
        a.list = (const uint32_t*)ctx->fb[ctx->cur].out_rows.p;
        a.list_base = (const uint64_t*)ctx->seg_bases.p + seg;
    }
    a.global = ctx->g;
    a.depth_bias = ctx->depth_bias;
    a.entity_keys = ctx->have_keys ? ctx->keys : nullptr;
    memcpy(a.row2, view_from_world_row2, sizeof a.row2);
    a.out_rows = (uint32_t*)ctx->ps_rows.p;
    a.out_keys = (uint64_t*)ctx->ps_keys.p;
    a.out_distance = (float*)ctx->ps_dist.p;
    a.out_count = (uint32_t*)ctx->ps_count.p;
    HIP_TRY(ctx, launch_phase_sort(a, ctx->stream));
    ctx->ps_state = mi_ctx::PS_SORTED;
    return MI_OK;
}

int32_t mi_phase_sort_download(mi_ctx* ctx, uint32_t* out_rows, uint64_t* out_entity_keys, float* out_distance, uint32_t capacity,
                               uint32_t* out_count) {
    ENTER(ctx);
    if (!out_count) return fail(ctx, MI_ERR_INVALID_ARG, "mi_phase_sort_download: NULL out_count");
    if (ctx->ps_state == mi_ctx::PS_NONE) return fail(ctx, MI_ERR_NOT_READY, "mi_phase_sort_download before mi_phase_sort");
    uint32_t total = 0;
    int32_t rc;
    if (ctx->ps_state == mi_ctx::PS_SORTED && (rc = download(ctx, &total, ctx->ps_count.p, 4))) return rc;
    *out_count = total;
    if (total > capacity) return fail(ctx, MI_ERR_CAPACITY, "sorted phase has %u items, capacity %u", total, capacity);
    if (total == 0) return MI_OK;
    if (out_rows && (rc = download(ctx, out_rows, ctx->ps_rows.p, (size_t)total * 4))) return rc;
    if (out_entity_keys && (rc = download(ctx, out_entity_keys, ctx->ps_keys.p, (size_t)total * 8))) return rc;
    if (out_distance && (rc = download(ctx, out_distance, ctx->ps_dist.p, (size_t)total * 4))) return rc;
    return MI_OK;
}

}  // extern "C"
