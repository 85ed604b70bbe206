// ctx_anim.cpp -- animation clips: the entry points in front of kernels_anim.hip.  The two uploads check every index the kernel
// will follow (it tests none of them again) and lay the targets out for it; mi_anim_frame is one launch, and to the context's state
// what an indexed Transform upload of the same rows is (indexed_write_begin / _end, context.cpp).  The same pair for blended
// players: mi_anim_upload_blend_targets and mi_anim_frame_blended, which also checks and packs the frame's layers.  And a triple
// for whole animation graphs: mi_anim_upload_graphs compiles each tree into the program k_anim_graph runs, mi_anim_upload_graph_targets
// lays the targets out by graph, mi_anim_frame_graph hands the frame's node states over.  Morph weights run through the same graphs
// from a pool of weight tracks of their own: mi_anim_upload_weight_tracks, mi_anim_upload_morph_targets (which cuts the targets into
// the chunks k_anim_weights gives a wave each), mi_anim_frame_weights, mi_anim_download_weights.
#include "ctx.h"

using namespace mi;
using namespace mi_detail;

namespace {
uint32_t anim_width(uint32_t kind_interp) { return (kind_interp & ~ANIM_INTERP_MASK) == ANIM_ROTATION ? 4u : 3u; }
}  // namespace

extern "C" {

int32_t mi_anim_upload_tracks(mi_ctx* ctx, uint32_t n_tracks, const mi_anim_track* tracks, uint32_t n_times, const float* times, uint32_t n_values,
                              const float* values) {
    ENTER(ctx);
    if ((n_tracks && !tracks) || (n_times && !times) || (n_values && !values)) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_tracks: NULL array");
    // ---- validation: nothing of the previous pool is touched before it has passed ----
    for (uint32_t i = 0; i < n_tracks; ++i) {
        const mi_anim_track& tr = tracks[i];
        const uint32_t interp = tr.kind_interp & ANIM_INTERP_MASK, comp = tr.kind_interp & ~ANIM_INTERP_MASK;
        if (interp > ANIM_CUBIC) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_tracks: track %u: unknown interpolation in kind_interp 0x%x", i, tr.kind_interp);
        if (comp != ANIM_TRANSLATION && comp != ANIM_ROTATION && comp != ANIM_SCALE)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_tracks: track %u: unknown component in kind_interp 0x%x", i, tr.kind_interp);
        if (tr.n_keys == 0) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_tracks: track %u has no keys", i);
        if ((uint64_t)tr.first_time + tr.n_keys > n_times)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_tracks: track %u: times [%u,+%u) exceed %u", i, tr.first_time, tr.n_keys, n_times);
        const uint64_t floats = (uint64_t)tr.n_keys * anim_width(tr.kind_interp) * (interp == ANIM_CUBIC ? 3u : 1u);
        if ((uint64_t)tr.first_value + floats > n_values)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_tracks: track %u: values [%u,+%llu) exceed %u", i, tr.first_value, (unsigned long long)floats, n_values);
        const float* t = times + tr.first_time;
        for (uint32_t k = 1; k < tr.n_keys; ++k)
            if (!(t[k] > t[k - 1u])) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_tracks: track %u: times not strictly ascending at key %u", i, k);
    }
    int32_t rc;
    if ((rc = ensure(ctx, ctx->an_tracks, (size_t)n_tracks * sizeof(mi_anim_track)))) return rc;
    if ((rc = ensure(ctx, ctx->an_times, (size_t)n_times * 4))) return rc;
    if ((rc = ensure(ctx, ctx->an_values, (size_t)n_values * 4))) return rc;
    ctx->an_have_tracks = ctx->an_have_targets = ctx->an_have_blend_targets = ctx->an_have_graph_targets = false;
    if ((rc = upload(ctx, ctx->an_tracks.p, tracks, (size_t)n_tracks * sizeof(mi_anim_track)))) return rc;
    if ((rc = upload(ctx, ctx->an_times.p, times, (size_t)n_times * 4))) return rc;
    if ((rc = upload(ctx, ctx->an_values.p, values, (size_t)n_values * 4))) return rc;
    ctx->an_tracks_host.assign(tracks, tracks + n_tracks);
    ctx->an_n_targets = ctx->an_bl_n_targets = ctx->an_gr_n_targets = 0;
    ctx->an_have_tracks = true;
    return MI_OK;
}

int32_t mi_anim_upload_targets(mi_ctx* ctx, uint32_t n_targets, const mi_anim_target* targets) {
    ENTER(ctx);
    if (n_targets && !targets) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_targets: NULL");
    if (!ctx->an_have_tracks) return fail(ctx, MI_ERR_NOT_READY, "mi_anim_upload_targets before mi_anim_upload_tracks");
    // ---- validation: nothing of the previous targets is touched before it has passed ----
    const std::vector<mi_anim_track>& pool = ctx->an_tracks_host;
    static const char* const field[3] = {"track_t", "track_r", "track_s"};
    static const uint32_t comp_of[3] = {ANIM_TRANSLATION, ANIM_ROTATION, ANIM_SCALE};
    uint32_t row_end = 0, player_end = 0, scale_lo = 0xFFFFFFFFu, scale_hi = 0;
    for (uint32_t i = 0; i < n_targets; ++i) {
        const mi_anim_target& tg = targets[i];
        if (tg.row >= ctx->n) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_targets: target %u: row %u >= %u live rows", i, tg.row, ctx->n);
        if (tg.player == 0xFFFFFFFFu) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_targets: target %u: player 0x%x", i, tg.player);
        const uint32_t tr[3] = {tg.track_t, tg.track_r, tg.track_s};
        for (uint32_t c = 0; c < 3; ++c) {
            if (tr[c] == MI_ANIM_NO_TRACK) continue;
            if (tr[c] >= pool.size()) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_targets: target %u: %s %u >= %zu tracks", i, field[c], tr[c], pool.size());
            if ((pool[tr[c]].kind_interp & ~ANIM_INTERP_MASK) != comp_of[c])
                return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_targets: target %u: %s %u is a track of another component (kind_interp 0x%x)", i, field[c], tr[c],
                            pool[tr[c]].kind_interp);
        }
        row_end = std::max(row_end, tg.row + 1u);
        player_end = std::max(player_end, tg.player + 1u);
        if (tg.track_s != MI_ANIM_NO_TRACK) scale_lo = std::min(scale_lo, tg.row), scale_hi = std::max(scale_hi, tg.row);
    }
    // ---- the launch order: by player, by row (rows are distinct: adjacent equals after the sort are the duplicates) ----
    std::vector<uint32_t> order(n_targets);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return targets[x].row < targets[y].row; });
    for (uint32_t i = 1; i < n_targets; ++i)
        if (targets[order[i]].row == targets[order[i - 1u]].row) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_targets: row %u belongs to two targets", targets[order[i]].row);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return targets[x].player < targets[y].player; });
    std::vector<uint32_t> soa((size_t)5 * n_targets);
    const uint32_t n_wgs = (n_targets + ANIM_THREADS - 1u) / ANIM_THREADS;
    std::vector<uint32_t> wg_times((size_t)2 * n_wgs, 0u);
    for (uint32_t w = 0; w < n_wgs; ++w) {
        uint64_t lo = UINT64_MAX, hi = 0;  // the range of key times this workgroup's tracks use
        for (uint32_t i = w * ANIM_THREADS; i < std::min(n_targets, (w + 1u) * ANIM_THREADS); ++i) {
            const mi_anim_target& tg = targets[order[i]];
            const uint32_t col[5] = {tg.row, tg.player, tg.track_t, tg.track_r, tg.track_s};
            for (uint32_t c = 0; c < 5; ++c) soa[(size_t)c * n_targets + i] = col[c];
            for (uint32_t c = 2; c < 5; ++c) {
                if (col[c] == MI_ANIM_NO_TRACK) continue;
                lo = std::min<uint64_t>(lo, pool[col[c]].first_time);
                hi = std::max<uint64_t>(hi, (uint64_t)pool[col[c]].first_time + pool[col[c]].n_keys);
            }
        }
        if (lo < hi && hi - lo <= ANIM_LDS_TIMES) wg_times[2u * w] = (uint32_t)lo, wg_times[2u * w + 1u] = (uint32_t)(hi - lo);
    }
    int32_t rc;
    if ((rc = ensure(ctx, ctx->an_targets, soa.size() * 4))) return rc;
    if ((rc = ensure(ctx, ctx->an_wg_times, wg_times.size() * 4))) return rc;
    ctx->an_have_targets = false;
    if ((rc = upload(ctx, ctx->an_targets.p, soa.data(), soa.size() * 4))) return rc;
    if ((rc = upload(ctx, ctx->an_wg_times.p, wg_times.data(), wg_times.size() * 4))) return rc;
    ctx->an_n_targets = n_targets;
    ctx->an_row_end = row_end;
    ctx->an_player_end = player_end;
    ctx->an_any_scale = scale_lo <= scale_hi;
    ctx->an_scale_lo = ctx->an_any_scale ? scale_lo : 0u;
    ctx->an_scale_hi = scale_hi;
    ctx->an_have_targets = true;
    return MI_OK;
}

int32_t mi_anim_frame(mi_ctx* ctx, uint32_t n_players, const float* seek_time, uint32_t flags) {
    ENTER(ctx);
    if (flags) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame: flags 0x%x", flags);
    if (!ctx->an_have_tracks || !ctx->an_have_targets) return fail(ctx, MI_ERR_NOT_READY, "mi_anim_frame before mi_anim_upload_tracks and mi_anim_upload_targets");
    if (ctx->an_row_end > ctx->n)
        return fail(ctx, MI_ERR_NOT_READY, "mi_anim_frame: the targets write row %u, the context has %u rows (upload the targets again)", ctx->an_row_end - 1u, ctx->n);
    if (ctx->an_player_end > n_players) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame: a target names player %u, n_players = %u", ctx->an_player_end - 1u, n_players);
    if (ctx->an_n_targets == 0) return MI_OK;
    if (!seek_time) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame: NULL");
    void *st = nullptr, *d_seek = nullptr;
    int32_t rc = stage_alloc(ctx, (size_t)n_players * 4, &st);
    if (rc) return rc;
    memcpy(st, seek_time, (size_t)n_players * 4);
    HIP_TRY(ctx, hipHostGetDevicePointer(&d_seek, st, 0));
    IndexedWrite w{};
    if ((rc = indexed_write_begin(ctx, &w))) return rc;
    if (ctx->an_any_scale) row_summary_touch(ctx, ROWSUM_PART_SCALE, ctx->an_scale_lo, ctx->an_scale_hi - ctx->an_scale_lo + 1u);
    AnimArgs a{};
    a.n_targets = ctx->an_n_targets;
    a.targets = (const uint32_t*)ctx->an_targets.p;
    a.wg_times = (const uint32_t*)ctx->an_wg_times.p;
    a.tracks = (const uint32_t*)ctx->an_tracks.p;
    a.times = (const float*)ctx->an_times.p;
    a.values = (const float*)ctx->an_values.p;
    a.seek = (const float*)d_seek;
    a.t = ctx->t, a.r = ctx->r, a.s = ctx->s;
    a.changed = ctx->changed;
    a.changed_gen = ctx->changed_gen;
    a.parent_idx = w.parent_idx;
    a.mark_bytes = w.mark_cur;
    a.clear_words = w.clear_other;
    a.n_clear_words = w.n_clear_words;
    a.anc = w.anc;
    HIP_TRY(ctx, launch_anim_frame(a, ctx->stream));
    indexed_write_end(ctx, w, ctx->an_n_targets);
    return MI_OK;
}

int32_t mi_anim_upload_blend_targets(mi_ctx* ctx, uint32_t n_targets, const mi_anim_blend_target* targets, uint32_t n_bindings, const mi_anim_binding* bindings) {
    ENTER(ctx);
    if ((n_targets && !targets) || (n_bindings && !bindings)) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_blend_targets: NULL array");
    if (!ctx->an_have_tracks) return fail(ctx, MI_ERR_NOT_READY, "mi_anim_upload_blend_targets before mi_anim_upload_tracks");
    // ---- validation: nothing of the previous blended targets is touched before it has passed ----
    const std::vector<mi_anim_track>& pool = ctx->an_tracks_host;
    static const char* const field[3] = {"track_t", "track_r", "track_s"};
    static const uint32_t comp_of[3] = {ANIM_TRANSLATION, ANIM_ROTATION, ANIM_SCALE};
    uint32_t row_end = 0, player_end = 0, scale_lo = 0xFFFFFFFFu, scale_hi = 0;
    for (uint32_t i = 0; i < n_targets; ++i) {
        const mi_anim_blend_target& tg = targets[i];
        if (tg.row >= ctx->n) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_blend_targets: target %u: row %u >= %u live rows", i, tg.row, ctx->n);
        if (tg.player == 0xFFFFFFFFu) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_blend_targets: target %u: player 0x%x", i, tg.player);
        if (tg.n_clips == 0) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_blend_targets: target %u has no clips", i);
        if ((uint64_t)tg.first_binding + tg.n_clips > n_bindings)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_blend_targets: target %u: bindings [%u,+%u) exceed %u", i, tg.first_binding, tg.n_clips, n_bindings);
        for (uint32_t c = 0; c < tg.n_clips; ++c) {
            const mi_anim_binding& bd = bindings[tg.first_binding + c];
            const uint32_t tr[3] = {bd.track_t, bd.track_r, bd.track_s};
            for (uint32_t k = 0; k < 3; ++k) {
                if (tr[k] == MI_ANIM_NO_TRACK) continue;
                if (tr[k] >= pool.size())
                    return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_blend_targets: target %u, clip %u: %s %u >= %zu tracks", i, c, field[k], tr[k], pool.size());
                if ((pool[tr[k]].kind_interp & ~ANIM_INTERP_MASK) != comp_of[k])
                    return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_blend_targets: target %u, clip %u: %s %u is a track of another component (kind_interp 0x%x)", i, c,
                                field[k], tr[k], pool[tr[k]].kind_interp);
            }
            if (bd.track_s != MI_ANIM_NO_TRACK) scale_lo = std::min(scale_lo, tg.row), scale_hi = std::max(scale_hi, tg.row);
        }
        row_end = std::max(row_end, tg.row + 1u);
        player_end = std::max(player_end, tg.player + 1u);
    }
    // ---- the launch order, as mi_anim_upload_targets: by player, by row ----
    std::vector<uint32_t> order(n_targets);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return targets[x].row < targets[y].row; });
    for (uint32_t i = 1; i < n_targets; ++i)
        if (targets[order[i]].row == targets[order[i - 1u]].row)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_blend_targets: row %u belongs to two targets", targets[order[i]].row);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return targets[x].player < targets[y].player; });
    // ---- per player: its targets [g0, g1) of the order, the smallest n_clips among them, and its block of the re-laid bindings
    // ---- (kernels.h, AnimBlendArgs: [clip][component][target of the player])
    std::vector<uint32_t> players, clips, count, soa((size_t)4 * n_targets), relaid;
    std::vector<uint32_t> reach(n_targets);  // the clips of a target a layer can name: its player's smallest n_clips
    for (uint32_t g0 = 0, g1; g0 < n_targets; g0 = g1) {
        const uint32_t player = targets[order[g0]].player;
        uint32_t c_min = 0xFFFFFFFFu;
        for (g1 = g0; g1 < n_targets && targets[order[g1]].player == player; ++g1) c_min = std::min(c_min, targets[order[g1]].n_clips);
        const uint32_t t_n = g1 - g0;
        const uint64_t block = relaid.size();
        if (block + (uint64_t)3 * c_min * t_n > 0xFFFFFFFFull) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_blend_targets: more than 2^32 binding words");
        relaid.resize((size_t)(block + (uint64_t)3 * c_min * t_n));
        for (uint32_t j = 0; j < t_n; ++j) {
            const mi_anim_blend_target& tg = targets[order[g0 + j]];
            const uint32_t col[4] = {tg.row, tg.player, (uint32_t)block + j, t_n};
            for (uint32_t c = 0; c < 4; ++c) soa[(size_t)c * n_targets + g0 + j] = col[c];
            reach[g0 + j] = c_min;
            for (uint32_t c = 0; c < c_min; ++c) {
                const mi_anim_binding& bd = bindings[tg.first_binding + c];
                const uint32_t tr[3] = {bd.track_t, bd.track_r, bd.track_s};
                for (uint32_t k = 0; k < 3; ++k) relaid[(size_t)block + (size_t)(3u * c + k) * t_n + j] = tr[k];
            }
        }
        players.push_back(player), clips.push_back(c_min), count.push_back(t_n);
    }
    const uint32_t n_wgs = (n_targets + ANIM_BLEND_TARGETS - 1u) / ANIM_BLEND_TARGETS;
    std::vector<uint32_t> wg_times((size_t)2 * n_wgs, 0u);
    for (uint32_t w = 0; w < n_wgs; ++w) {
        uint64_t lo = UINT64_MAX, hi = 0;  // the range of key times the tracks within this workgroup's reach use
        for (uint32_t i = w * ANIM_BLEND_TARGETS; i < std::min(n_targets, (w + 1u) * ANIM_BLEND_TARGETS); ++i)
            for (uint32_t e = 0; e < 3u * reach[i]; ++e) {
                const uint32_t tr = relaid[(size_t)soa[(size_t)2 * n_targets + i] + (size_t)e * soa[(size_t)3 * n_targets + i]];
                if (tr == MI_ANIM_NO_TRACK) continue;
                lo = std::min<uint64_t>(lo, pool[tr].first_time);
                hi = std::max<uint64_t>(hi, (uint64_t)pool[tr].first_time + pool[tr].n_keys);
            }
        if (lo < hi && hi - lo <= ANIM_LDS_TIMES) wg_times[2u * w] = (uint32_t)lo, wg_times[2u * w + 1u] = (uint32_t)(hi - lo);
    }
    int32_t rc;
    if ((rc = ensure(ctx, ctx->an_bl_targets, soa.size() * 4))) return rc;
    if ((rc = ensure(ctx, ctx->an_bl_bindings, relaid.size() * 4))) return rc;
    if ((rc = ensure(ctx, ctx->an_bl_wg_times, wg_times.size() * 4))) return rc;
    ctx->an_have_blend_targets = false;
    if ((rc = upload(ctx, ctx->an_bl_targets.p, soa.data(), soa.size() * 4))) return rc;
    if ((rc = upload(ctx, ctx->an_bl_bindings.p, relaid.data(), relaid.size() * 4))) return rc;
    if ((rc = upload(ctx, ctx->an_bl_wg_times.p, wg_times.data(), wg_times.size() * 4))) return rc;
    ctx->an_bl_players.swap(players), ctx->an_bl_clips.swap(clips), ctx->an_bl_count.swap(count);
    ctx->an_bl_n_targets = n_targets;
    ctx->an_bl_row_end = row_end;
    ctx->an_bl_player_end = player_end;
    ctx->an_bl_any_scale = scale_lo <= scale_hi;
    ctx->an_bl_scale_lo = ctx->an_bl_any_scale ? scale_lo : 0u;
    ctx->an_bl_scale_hi = scale_hi;
    ctx->an_have_blend_targets = true;
    return MI_OK;
}

int32_t mi_anim_frame_blended(mi_ctx* ctx, uint32_t n_players, uint32_t n_layers, const mi_anim_layer* layers, uint32_t flags) {
    ENTER(ctx);
    if (flags) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_blended: flags 0x%x", flags);
    if (!ctx->an_have_tracks || !ctx->an_have_blend_targets)
        return fail(ctx, MI_ERR_NOT_READY, "mi_anim_frame_blended before mi_anim_upload_tracks and mi_anim_upload_blend_targets");
    if (ctx->an_bl_row_end > ctx->n)
        return fail(ctx, MI_ERR_NOT_READY, "mi_anim_frame_blended: the targets write row %u, the context has %u rows (upload the targets again)", ctx->an_bl_row_end - 1u,
                    ctx->n);
    if (ctx->an_bl_player_end > n_players)
        return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_blended: a target names player %u, n_players = %u", ctx->an_bl_player_end - 1u, n_players);
    if (n_layers && !layers) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_blended: NULL");
    // ---- the layers the kernel will see: weight > 0, of players that have targets (an_bl_players ascends, as the layers' players must)
    std::vector<uint32_t> kept;
    const std::vector<uint32_t>& players = ctx->an_bl_players;
    size_t cur = 0;
    uint32_t of_player = 0, rows = 0;  // kept layers of players[cur] so far; targets of the players with kept layers
    for (uint32_t i = 0; i < n_layers; ++i) {
        const mi_anim_layer& ly = layers[i];
        if (i && ly.player < layers[i - 1u].player)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_blended: layer %u: player %u behind player %u (layers go by player, ascending)", i, ly.player, layers[i - 1u].player);
        if (ly.player >= n_players) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_blended: layer %u: player %u >= n_players = %u", i, ly.player, n_players);
        if (!(ly.weight > 0.0f)) continue;  // (zero, negative, NaN)
        while (cur < players.size() && players[cur] < ly.player) ++cur, of_player = 0;
        if (cur == players.size() || players[cur] != ly.player) continue;  // (a player without blended targets: nothing to write)
        if (ly.clip >= ctx->an_bl_clips[cur])
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_blended: layer %u: clip %u, a target of player %u has %u clips", i, ly.clip, ly.player, ctx->an_bl_clips[cur]);
        if (++of_player > MI_ANIM_MAX_LAYERS)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_blended: player %u has more than %u layers of weight > 0", ly.player, MI_ANIM_MAX_LAYERS);
        if (of_player == 1u) rows += ctx->an_bl_count[cur];
        kept.push_back(i);
    }
    if (kept.empty()) return MI_OK;  // every player is left alone
    if (kept.size() >> ANIM_BLEND_COUNT_SHIFT) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_blended: %zu layers", kept.size());
    // ---- one word per player and 12 bytes per kept layer, in the pinned staging block: the kernel reads them where they are ----
    void *st = nullptr, *d_st = nullptr;
    int32_t rc = stage_alloc(ctx, ((size_t)n_players + 3u * kept.size()) * 4, &st);
    if (rc) return rc;
    uint32_t *words = (uint32_t*)st, *packed = words + n_players;
    memset(words, 0, (size_t)n_players * 4);
    for (size_t k = 0; k < kept.size(); ++k) {
        const mi_anim_layer& ly = layers[kept[k]];
        if (!words[ly.player]) words[ly.player] = (uint32_t)k;
        words[ly.player] += 1u << ANIM_BLEND_COUNT_SHIFT;
        packed[3u * k] = ly.clip;
        memcpy(packed + 3u * k + 1u, &ly.seek_time, 8);  // seek_time, weight
    }
    HIP_TRY(ctx, hipHostGetDevicePointer(&d_st, st, 0));
    IndexedWrite w{};
    if ((rc = indexed_write_begin(ctx, &w))) return rc;
    if (ctx->an_bl_any_scale) row_summary_touch(ctx, ROWSUM_PART_SCALE, ctx->an_bl_scale_lo, ctx->an_bl_scale_hi - ctx->an_bl_scale_lo + 1u);
    AnimBlendArgs a{};
    a.n_targets = ctx->an_bl_n_targets;
    a.targets = (const uint32_t*)ctx->an_bl_targets.p;
    a.bindings = (const uint32_t*)ctx->an_bl_bindings.p;
    a.wg_times = (const uint32_t*)ctx->an_bl_wg_times.p;
    a.tracks = (const uint32_t*)ctx->an_tracks.p;
    a.times = (const float*)ctx->an_times.p;
    a.values = (const float*)ctx->an_values.p;
    a.players = (const uint32_t*)d_st;
    a.layers = (const uint32_t*)d_st + n_players;
    a.t = ctx->t, a.r = ctx->r, a.s = ctx->s;
    a.changed = ctx->changed;
    a.changed_gen = ctx->changed_gen;
    a.parent_idx = w.parent_idx;
    a.mark_bytes = w.mark_cur;
    a.clear_words = w.clear_other;
    a.n_clear_words = w.n_clear_words;
    a.anc = w.anc;
    HIP_TRY(ctx, launch_anim_blend(a, ctx->stream));
    indexed_write_end(ctx, w, rows);
    return MI_OK;
}

int32_t mi_anim_upload_graphs(mi_ctx* ctx, uint32_t n_graphs, const mi_anim_graph* graphs, uint32_t n_nodes, const mi_anim_graph_node* nodes) {
    ENTER(ctx);
    if ((n_graphs && !graphs) || (n_nodes && !nodes)) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graphs: NULL array");
    // ---- validation and compilation: nothing of the previous graphs is touched before every graph has passed ----
    std::vector<uint32_t> prog, prog_first(n_graphs), prog_n(n_graphs);
    for (uint32_t gi = 0; gi < n_graphs; ++gi) {
        const mi_anim_graph& gr = graphs[gi];
        if (gr.n_nodes == 0 || gr.n_nodes > MI_ANIM_MAX_GRAPH_NODES)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graphs: graph %u has %u nodes (1 .. %u)", gi, gr.n_nodes, MI_ANIM_MAX_GRAPH_NODES);
        if ((uint64_t)gr.first_node + gr.n_nodes > n_nodes)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graphs: graph %u: nodes [%u,+%u) exceed %u", gi, gr.first_node, gr.n_nodes, n_nodes);
        const mi_anim_graph_node* nd = nodes + gr.first_node;
        uint32_t depth[ANIM_GRAPH_MAX_NODES];
        uint64_t eff[ANIM_GRAPH_MAX_NODES];
        std::vector<uint32_t> kids[ANIM_GRAPH_MAX_NODES];
        for (uint32_t k = 0; k < gr.n_nodes; ++k) {
            if (nd[k].kind > MI_ANIM_NODE_ADD) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graphs: graph %u, node %u: unknown kind %u", gi, k, nd[k].kind);
            const uint64_t own = (uint64_t)nd[k].mask_lo | (uint64_t)nd[k].mask_hi << 32;
            if (k == 0) {
                if (nd[0].parent != MI_ANIM_NO_NODE) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graphs: graph %u: node 0 is the root, its parent is %u", gi, nd[0].parent);
                depth[0] = 1u, eff[0] = own;
                continue;
            }
            const uint32_t p = nd[k].parent;
            if (p == MI_ANIM_NO_NODE) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graphs: graph %u: node %u is a second root", gi, k);
            if (p >= k) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graphs: graph %u, node %u: parent %u is not below it", gi, k, p);
            if (nd[p].kind == MI_ANIM_NODE_CLIP) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graphs: graph %u, node %u: its parent %u is a clip node", gi, k, p);
            depth[k] = depth[p] + 1u, eff[k] = own | eff[p];
            if (depth[k] > MI_ANIM_MAX_GRAPH_DEPTH)
                return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graphs: graph %u, node %u: depth %u (the root is 1, the most %u)", gi, k, depth[k], MI_ANIM_MAX_GRAPH_DEPTH);
            kids[p].push_back(k);
        }
        // ---- the program (kernels.h, AnimGraphArgs): pre-order, children by ascending index; an inner node without children emits nothing
        prog_first[gi] = (uint32_t)(prog.size() / 4u);
        struct Open { uint32_t node, next, enter; };  // an entered inner node: its next child, and where its ENTER stands
        std::vector<Open> open;
        auto emit = [&](uint32_t op, uint32_t k, uint32_t clip) {
            const uint32_t into = k ? nd[nd[k].parent].kind : (uint32_t)MI_ANIM_NODE_BLEND;  // (the root is the result's first and only child)
            prog.insert(prog.end(), {op | depth[k] << 2 | into << 6 | k << 8, clip, (uint32_t)eff[k], (uint32_t)(eff[k] >> 32)});
        };
        auto visit = [&](uint32_t k) {
            if (nd[k].kind == MI_ANIM_NODE_CLIP) emit(ANIM_OP_CLIP, k, nd[k].clip);
            else if (!kids[k].empty()) open.push_back({k, 0u, (uint32_t)(prog.size() / 4u)}), emit(ANIM_OP_ENTER, k, 0u);
        };
        visit(0u);
        while (!open.empty()) {
            Open& o = open.back();
            if (o.next < kids[o.node].size()) {
                visit(kids[o.node][o.next++]);  // (may grow `open`: o is not used behind it)
                continue;
            }
            emit(ANIM_OP_LEAVE, o.node, 0u);
            prog[4u * (size_t)o.enter] |= ((uint32_t)(prog.size() / 4u) - o.enter) << 16;  // skip: to behind the LEAVE
            open.pop_back();
        }
        prog_n[gi] = (uint32_t)(prog.size() / 4u) - prog_first[gi];
    }
    int32_t rc;
    if ((rc = ensure(ctx, ctx->an_gr_prog, prog.size() * 4))) return rc;
    ctx->an_have_graphs = ctx->an_have_graph_targets = ctx->an_have_morph_targets = false;
    if ((rc = upload(ctx, ctx->an_gr_prog.p, prog.data(), prog.size() * 4))) return rc;
    ctx->an_gr_graphs.assign(graphs, graphs + n_graphs);
    ctx->an_gr_nodes.assign(nodes, nodes + n_nodes);
    ctx->an_gr_prog_first.swap(prog_first), ctx->an_gr_prog_n.swap(prog_n);
    ctx->an_gr_n_targets = ctx->an_mw_n_chunks = 0;
    ctx->an_have_graphs = true;
    return MI_OK;
}

int32_t mi_anim_upload_graph_targets(mi_ctx* ctx, uint32_t n_targets, const mi_anim_graph_target* targets, uint32_t n_bindings, const mi_anim_binding* bindings,
                                     uint32_t n_players, const uint32_t* player_graph) {
    ENTER(ctx);
    if ((n_targets && !targets) || (n_bindings && !bindings) || (n_players && !player_graph))
        return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graph_targets: NULL array");
    if (!ctx->an_have_tracks || !ctx->an_have_graphs)
        return fail(ctx, MI_ERR_NOT_READY, "mi_anim_upload_graph_targets before mi_anim_upload_tracks and mi_anim_upload_graphs");
    // ---- validation: nothing of the previous graph targets is touched before it has passed ----
    const std::vector<mi_anim_track>& pool = ctx->an_tracks_host;
    static const char* const field[3] = {"track_t", "track_r", "track_s"};
    static const uint32_t comp_of[3] = {ANIM_TRANSLATION, ANIM_ROTATION, ANIM_SCALE};
    for (uint32_t p = 0; p < n_players; ++p)
        if (player_graph[p] != MI_ANIM_NO_NODE && player_graph[p] >= ctx->an_gr_graphs.size())
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graph_targets: player %u: graph %u >= %zu graphs", p, player_graph[p], ctx->an_gr_graphs.size());
    uint32_t row_end = 0, player_end = 0, scale_lo = 0xFFFFFFFFu, scale_hi = 0;
    std::vector<uint32_t> c_min(n_players, 0xFFFFFFFFu), count(n_players, 0u);  // per player: the smallest n_clips of its targets; its targets
    for (uint32_t i = 0; i < n_targets; ++i) {
        const mi_anim_graph_target& tg = targets[i];
        if (tg.row >= ctx->n) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graph_targets: target %u: row %u >= %u live rows", i, tg.row, ctx->n);
        if (tg.player >= n_players) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graph_targets: target %u: player %u >= n_players = %u", i, tg.player, n_players);
        if (player_graph[tg.player] == MI_ANIM_NO_NODE) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graph_targets: target %u: player %u has no graph", i, tg.player);
        if (tg.n_clips == 0) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graph_targets: target %u has no clips", i);
        if ((uint64_t)tg.first_binding + tg.n_clips > n_bindings)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graph_targets: target %u: bindings [%u,+%u) exceed %u", i, tg.first_binding, tg.n_clips, n_bindings);
        for (uint32_t c = 0; c < tg.n_clips; ++c) {
            const mi_anim_binding& bd = bindings[tg.first_binding + c];
            const uint32_t tr[3] = {bd.track_t, bd.track_r, bd.track_s};
            for (uint32_t k = 0; k < 3; ++k) {
                if (tr[k] == MI_ANIM_NO_TRACK) continue;
                if (tr[k] >= pool.size())
                    return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graph_targets: target %u, clip %u: %s %u >= %zu tracks", i, c, field[k], tr[k], pool.size());
                if ((pool[tr[k]].kind_interp & ~ANIM_INTERP_MASK) != comp_of[k])
                    return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graph_targets: target %u, clip %u: %s %u is a track of another component (kind_interp 0x%x)", i, c,
                                field[k], tr[k], pool[tr[k]].kind_interp);
            }
            if (bd.track_s != MI_ANIM_NO_TRACK) scale_lo = std::min(scale_lo, tg.row), scale_hi = std::max(scale_hi, tg.row);
        }
        row_end = std::max(row_end, tg.row + 1u);
        player_end = std::max(player_end, tg.player + 1u);
        c_min[tg.player] = std::min(c_min[tg.player], tg.n_clips), ++count[tg.player];
    }
    for (uint32_t p = 0; p < n_players; ++p) {
        if (!count[p]) continue;
        const mi_anim_graph& gr = ctx->an_gr_graphs[player_graph[p]];
        for (uint32_t k = 0; k < gr.n_nodes; ++k) {
            const mi_anim_graph_node& nd = ctx->an_gr_nodes[gr.first_node + k];
            if (nd.kind == MI_ANIM_NODE_CLIP && nd.clip >= c_min[p])
                return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graph_targets: graph %u, node %u: clip %u, a target of player %u has %u clips", player_graph[p], k, nd.clip, p,
                            c_min[p]);
        }
    }
    // ---- the launch order: by graph, by player, by row; a graph's targets start a workgroup of their own ----
    std::vector<uint32_t> order(n_targets);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return targets[x].row < targets[y].row; });
    for (uint32_t i = 1; i < n_targets; ++i)
        if (targets[order[i]].row == targets[order[i - 1u]].row)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graph_targets: row %u belongs to two targets", targets[order[i]].row);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        const mi_anim_graph_target &a = targets[x], &b = targets[y];
        return player_graph[a.player] != player_graph[b.player] ? player_graph[a.player] < player_graph[b.player] : a.player < b.player;
    });
    std::vector<uint32_t> slot(n_targets);  // where target order[i] stands among the padded targets
    uint64_t n_padded = 0;
    for (uint32_t i = 0; i < n_targets; ++i) {
        if (i && player_graph[targets[order[i]].player] != player_graph[targets[order[i - 1u]].player])
            n_padded = (n_padded + ANIM_GRAPH_TARGETS - 1u) / ANIM_GRAPH_TARGETS * ANIM_GRAPH_TARGETS;
        slot[i] = (uint32_t)n_padded++;
    }
    n_padded = (n_padded + ANIM_GRAPH_TARGETS - 1u) / ANIM_GRAPH_TARGETS * ANIM_GRAPH_TARGETS;
    if (n_padded > 0x7FFFFFFFull) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graph_targets: %u targets", n_targets);
    const size_t np = (size_t)n_padded;
    std::vector<uint32_t> soa(6 * np, 0u), relaid;
    std::fill(soa.begin(), soa.begin() + np, ANIM_GRAPH_NO_NODE);  // (rows of the padding)
    const uint32_t n_wgs = (uint32_t)(np / ANIM_GRAPH_TARGETS);
    std::vector<uint32_t> wg((size_t)4 * n_wgs, 0u);
    std::vector<uint64_t> t_lo(n_wgs, UINT64_MAX), t_hi(n_wgs, 0);  // per workgroup: the range of key times the tracks within its reach use
    for (uint32_t g0 = 0, g1; g0 < n_targets; g0 = g1) {  // per player, as mi_anim_upload_blend_targets: its block of the re-laid bindings
        const uint32_t player = targets[order[g0]].player, clips = c_min[player];
        for (g1 = g0; g1 < n_targets && targets[order[g1]].player == player; ++g1) {}
        const uint32_t t_n = g1 - g0;
        const uint64_t block = relaid.size();
        if (block + (uint64_t)3 * clips * t_n > 0xFFFFFFFFull) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_graph_targets: more than 2^32 binding words");
        relaid.resize((size_t)(block + (uint64_t)3 * clips * t_n));
        for (uint32_t j = 0; j < t_n; ++j) {
            const mi_anim_graph_target& tg = targets[order[g0 + j]];
            const uint32_t at = slot[g0 + j], w = at / ANIM_GRAPH_TARGETS;
            const uint32_t col[6] = {tg.row, tg.player, (uint32_t)block + j, t_n, tg.groups_lo, tg.groups_hi};
            for (uint32_t c = 0; c < 6; ++c) soa[c * np + at] = col[c];
            wg[4u * w + 2u] = ctx->an_gr_prog_first[player_graph[player]], wg[4u * w + 3u] = ctx->an_gr_prog_n[player_graph[player]];
            for (uint32_t c = 0; c < clips; ++c) {
                const mi_anim_binding& bd = bindings[tg.first_binding + c];
                const uint32_t tr[3] = {bd.track_t, bd.track_r, bd.track_s};
                for (uint32_t k = 0; k < 3; ++k) {
                    relaid[(size_t)block + (size_t)(3u * c + k) * t_n + j] = tr[k];
                    if (tr[k] == MI_ANIM_NO_TRACK) continue;
                    t_lo[w] = std::min<uint64_t>(t_lo[w], pool[tr[k]].first_time);
                    t_hi[w] = std::max<uint64_t>(t_hi[w], (uint64_t)pool[tr[k]].first_time + pool[tr[k]].n_keys);
                }
            }
        }
    }
    for (uint32_t w = 0; w < n_wgs; ++w)
        if (t_lo[w] < t_hi[w] && t_hi[w] - t_lo[w] <= ANIM_LDS_TIMES) wg[4u * w] = (uint32_t)t_lo[w], wg[4u * w + 1u] = (uint32_t)(t_hi[w] - t_lo[w]);
    int32_t rc;
    if ((rc = ensure(ctx, ctx->an_gr_targets, soa.size() * 4))) return rc;
    if ((rc = ensure(ctx, ctx->an_gr_bindings, relaid.size() * 4))) return rc;
    if ((rc = ensure(ctx, ctx->an_gr_wg, wg.size() * 4))) return rc;
    ctx->an_have_graph_targets = false;
    if ((rc = upload(ctx, ctx->an_gr_targets.p, soa.data(), soa.size() * 4))) return rc;
    if ((rc = upload(ctx, ctx->an_gr_bindings.p, relaid.data(), relaid.size() * 4))) return rc;
    if ((rc = upload(ctx, ctx->an_gr_wg.p, wg.data(), wg.size() * 4))) return rc;
    ctx->an_gr_player_graph.assign(player_graph, player_graph + n_players);
    ctx->an_gr_player_count.swap(count);
    ctx->an_gr_n_targets = (uint32_t)np;
    ctx->an_gr_row_end = row_end;
    ctx->an_gr_player_end = player_end;
    ctx->an_gr_any_scale = scale_lo <= scale_hi;
    ctx->an_gr_scale_lo = ctx->an_gr_any_scale ? scale_lo : 0u;
    ctx->an_gr_scale_hi = scale_hi;
    ctx->an_have_graph_targets = true;
    return MI_OK;
}

int32_t mi_anim_frame_graph(mi_ctx* ctx, uint32_t n_players, const uint32_t* first_state, uint32_t n_states, const mi_anim_node_state* states, uint32_t flags) {
    ENTER(ctx);
    if (flags) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_graph: flags 0x%x", flags);
    if (!ctx->an_have_tracks || !ctx->an_have_graphs || !ctx->an_have_graph_targets)
        return fail(ctx, MI_ERR_NOT_READY, "mi_anim_frame_graph before mi_anim_upload_tracks, mi_anim_upload_graphs and mi_anim_upload_graph_targets");
    if (ctx->an_gr_row_end > ctx->n)
        return fail(ctx, MI_ERR_NOT_READY, "mi_anim_frame_graph: the targets write row %u, the context has %u rows (upload the targets again)", ctx->an_gr_row_end - 1u, ctx->n);
    if (ctx->an_gr_player_end > n_players)
        return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_graph: a target names player %u, n_players = %u", ctx->an_gr_player_end - 1u, n_players);
    if ((n_players && !first_state) || (n_states && !states)) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_graph: NULL");
    uint32_t rows = 0;  // targets of the players that run this frame
    for (uint32_t p = 0; p < n_players; ++p) {
        if (first_state[p] == MI_ANIM_NO_NODE) continue;
        if (p >= ctx->an_gr_player_graph.size() || ctx->an_gr_player_graph[p] == MI_ANIM_NO_NODE)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_graph: player %u has states and no graph", p);
        const uint32_t nodes = ctx->an_gr_graphs[ctx->an_gr_player_graph[p]].n_nodes;
        if ((uint64_t)first_state[p] + nodes > n_states)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_graph: player %u: states [%u,+%u) exceed %u", p, first_state[p], nodes, n_states);
        rows += ctx->an_gr_player_count[p];
    }
    if (rows == 0) return MI_OK;  // every player that has targets is left alone
    // ---- one word per player and 8 bytes per state, in the pinned staging block: the kernel reads them where they are ----
    void *st = nullptr, *d_st = nullptr;
    int32_t rc = stage_alloc(ctx, ((size_t)n_players + 2u * (size_t)n_states) * 4, &st);
    if (rc) return rc;
    memcpy(st, first_state, (size_t)n_players * 4);
    memcpy((uint32_t*)st + n_players, states, (size_t)n_states * 8);
    HIP_TRY(ctx, hipHostGetDevicePointer(&d_st, st, 0));
    IndexedWrite w{};
    if ((rc = indexed_write_begin(ctx, &w))) return rc;
    if (ctx->an_gr_any_scale) row_summary_touch(ctx, ROWSUM_PART_SCALE, ctx->an_gr_scale_lo, ctx->an_gr_scale_hi - ctx->an_gr_scale_lo + 1u);
    AnimGraphArgs a{};
    a.n_targets = ctx->an_gr_n_targets;
    a.targets = (const uint32_t*)ctx->an_gr_targets.p;
    a.bindings = (const uint32_t*)ctx->an_gr_bindings.p;
    a.wg = (const uint32_t*)ctx->an_gr_wg.p;
    a.prog = (const uint32_t*)ctx->an_gr_prog.p;
    a.tracks = (const uint32_t*)ctx->an_tracks.p;
    a.times = (const float*)ctx->an_times.p;
    a.values = (const float*)ctx->an_values.p;
    a.first_state = (const uint32_t*)d_st;
    a.states = (const uint32_t*)d_st + n_players;
    a.t = ctx->t, a.r = ctx->r, a.s = ctx->s;
    a.changed = ctx->changed;
    a.changed_gen = ctx->changed_gen;
    a.parent_idx = w.parent_idx;
    a.mark_bytes = w.mark_cur;
    a.clear_words = w.clear_other;
    a.n_clear_words = w.n_clear_words;
    a.anc = w.anc;
    HIP_TRY(ctx, launch_anim_graph(a, ctx->stream));
    indexed_write_end(ctx, w, rows);
    return MI_OK;
}

int32_t mi_anim_upload_weight_tracks(mi_ctx* ctx, uint32_t n_tracks, const mi_anim_weight_track* tracks, uint32_t n_times, const float* times, uint32_t n_values,
                                     const float* values) {
    ENTER(ctx);
    if ((n_tracks && !tracks) || (n_times && !times) || (n_values && !values)) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_weight_tracks: NULL array");
    // ---- validation: nothing of the previous pool is touched before it has passed ----
    for (uint32_t i = 0; i < n_tracks; ++i) {
        const mi_anim_weight_track& tr = tracks[i];
        if (tr.interp > ANIM_CUBIC) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_weight_tracks: track %u: unknown interpolation %u", i, tr.interp);
        if (tr.n_keys == 0) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_weight_tracks: track %u has no keys", i);
        if (tr.n_weights == 0) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_weight_tracks: track %u has no weights", i);
        if ((uint64_t)tr.first_time + tr.n_keys > n_times)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_weight_tracks: track %u: times [%u,+%u) exceed %u", i, tr.first_time, tr.n_keys, n_times);
        const uint64_t per_key = (uint64_t)tr.n_weights * (tr.interp == ANIM_CUBIC ? 3u : 1u);  // (the product with n_keys may pass 2^64: divide instead)
        if (tr.first_value > n_values || tr.n_keys > (n_values - tr.first_value) / per_key)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_weight_tracks: track %u: values [%u,+%u x %llu) exceed %u", i, tr.first_value, tr.n_keys,
                        (unsigned long long)per_key, n_values);
        const float* t = times + tr.first_time;
        for (uint32_t k = 1; k < tr.n_keys; ++k)
            if (!(t[k] > t[k - 1u])) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_weight_tracks: track %u: times not strictly ascending at key %u", i, k);
    }
    int32_t rc;
    if ((rc = ensure(ctx, ctx->an_mw_tracks, (size_t)n_tracks * sizeof(mi_anim_weight_track)))) return rc;
    if ((rc = ensure(ctx, ctx->an_mw_times, (size_t)n_times * 4))) return rc;
    if ((rc = ensure(ctx, ctx->an_mw_values, (size_t)n_values * 4))) return rc;
    ctx->an_have_weight_tracks = ctx->an_have_morph_targets = false;
    if ((rc = upload(ctx, ctx->an_mw_tracks.p, tracks, (size_t)n_tracks * sizeof(mi_anim_weight_track)))) return rc;
    if ((rc = upload(ctx, ctx->an_mw_times.p, times, (size_t)n_times * 4))) return rc;
    if ((rc = upload(ctx, ctx->an_mw_values.p, values, (size_t)n_values * 4))) return rc;
    ctx->an_mw_tracks_host.assign(tracks, tracks + n_tracks);
    ctx->an_mw_n_chunks = 0;
    ctx->an_have_weight_tracks = true;
    return MI_OK;
}

int32_t mi_anim_upload_morph_targets(mi_ctx* ctx, uint32_t n_targets, const mi_anim_morph_target* targets, uint32_t n_bindings, const uint32_t* bindings,
                                     uint32_t n_players, const uint32_t* player_graph, uint32_t n_weights_out, const float* initial_weights) {
    ENTER(ctx);
    if ((n_targets && !targets) || (n_bindings && !bindings) || (n_players && !player_graph))
        return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_morph_targets: NULL array");
    if (!ctx->an_have_weight_tracks || !ctx->an_have_graphs)
        return fail(ctx, MI_ERR_NOT_READY, "mi_anim_upload_morph_targets before mi_anim_upload_weight_tracks and mi_anim_upload_graphs");
    // ---- validation: nothing of the previous morph targets or of their weights is touched before it has passed ----
    const std::vector<mi_anim_weight_track>& pool = ctx->an_mw_tracks_host;
    for (uint32_t p = 0; p < n_players; ++p)
        if (player_graph[p] != MI_ANIM_NO_NODE && player_graph[p] >= ctx->an_gr_graphs.size())
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_morph_targets: player %u: graph %u >= %zu graphs", p, player_graph[p], ctx->an_gr_graphs.size());
    uint32_t player_end = 0;
    uint64_t n_chunks = 0;
    std::vector<uint32_t> c_min(n_players, 0xFFFFFFFFu), count(n_players, 0u);  // per player: the smallest n_clips of its targets; its targets
    for (uint32_t i = 0; i < n_targets; ++i) {
        const mi_anim_morph_target& tg = targets[i];
        if (tg.n_weights == 0) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_morph_targets: target %u has no weights", i);
        if ((uint64_t)tg.first_weight + tg.n_weights > n_weights_out)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_morph_targets: target %u: weights [%u,+%u) exceed %u", i, tg.first_weight, tg.n_weights, n_weights_out);
        if (tg.player >= n_players) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_morph_targets: target %u: player %u >= n_players = %u", i, tg.player, n_players);
        if (player_graph[tg.player] == MI_ANIM_NO_NODE) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_morph_targets: target %u: player %u has no graph", i, tg.player);
        if (tg.n_clips == 0) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_morph_targets: target %u has no clips", i);
        if ((uint64_t)tg.first_binding + tg.n_clips > n_bindings)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_morph_targets: target %u: bindings [%u,+%u) exceed %u", i, tg.first_binding, tg.n_clips, n_bindings);
        for (uint32_t c = 0; c < tg.n_clips; ++c) {
            const uint32_t tr = bindings[tg.first_binding + c];
            if (tr == MI_ANIM_NO_TRACK) continue;
            if (tr >= pool.size()) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_morph_targets: target %u, clip %u: track %u >= %zu weight tracks", i, c, tr, pool.size());
            if (pool[tr].n_weights != tg.n_weights)
                return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_morph_targets: target %u, clip %u: track %u holds %u weights per key, the target has %u", i, c, tr,
                            pool[tr].n_weights, tg.n_weights);
        }
        player_end = std::max(player_end, tg.player + 1u);
        c_min[tg.player] = std::min(c_min[tg.player], tg.n_clips), ++count[tg.player];
        n_chunks += (tg.n_weights + ANIM_WEIGHT_LANES - 1u) / ANIM_WEIGHT_LANES;
    }
    if (n_chunks > 0x7FFFFFFFull) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_morph_targets: %llu blocks of 64 weights", (unsigned long long)n_chunks);
    for (uint32_t p = 0; p < n_players; ++p) {
        if (!count[p]) continue;
        const mi_anim_graph& gr = ctx->an_gr_graphs[player_graph[p]];
        for (uint32_t k = 0; k < gr.n_nodes; ++k) {
            const mi_anim_graph_node& nd = ctx->an_gr_nodes[gr.first_node + k];
            if (nd.kind == MI_ANIM_NODE_CLIP && nd.clip >= c_min[p])
                return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_morph_targets: graph %u, node %u: clip %u, a target of player %u has %u clips", player_graph[p], k, nd.clip, p,
                            c_min[p]);
        }
    }
    std::vector<uint32_t> order(n_targets);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return targets[x].first_weight < targets[y].first_weight; });
    for (uint32_t i = 1; i < n_targets; ++i) {  // (sorted by their first weight: two ranges overlap iff two neighbours do)
        const mi_anim_morph_target &a = targets[order[i - 1u]], &b = targets[order[i]];
        if ((uint64_t)a.first_weight + a.n_weights > b.first_weight)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_upload_morph_targets: targets %u and %u both write weight %u", order[i - 1u], order[i], b.first_weight);
    }
    // ---- the chunk table (kernels.h, AnimWeightArgs): by graph, by player, by first weight; a target's chunks by j0 ----
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        const mi_anim_morph_target &a = targets[x], &b = targets[y];
        return player_graph[a.player] != player_graph[b.player] ? player_graph[a.player] < player_graph[b.player] : a.player < b.player;
    });
    std::vector<uint32_t> chunks;
    chunks.reserve((size_t)n_chunks * ANIM_WEIGHT_CHUNK_WORDS);
    for (uint32_t i = 0; i < n_targets; ++i) {
        const mi_anim_morph_target& tg = targets[order[i]];
        const uint32_t g = player_graph[tg.player];
        for (uint64_t j = 0; j < tg.n_weights; j += ANIM_WEIGHT_LANES) {  // (64 bits: j0 + 64 may pass 2^32)
            const uint32_t j0 = (uint32_t)j;
            chunks.insert(chunks.end(), {tg.first_weight + j0, j0 | (std::min(tg.n_weights - j0, ANIM_WEIGHT_LANES) - 1u), ctx->an_gr_prog_first[g], ctx->an_gr_prog_n[g],
                                         tg.first_binding, tg.player, tg.groups_lo, tg.groups_hi});
        }
    }
    std::vector<float> zeros;
    if (!initial_weights) zeros.assign(n_weights_out, 0.0f);
    int32_t rc;
    if ((rc = ensure(ctx, ctx->an_mw_chunks, chunks.size() * 4))) return rc;
    if ((rc = ensure(ctx, ctx->an_mw_bindings, (size_t)n_bindings * 4))) return rc;
    if ((rc = ensure(ctx, ctx->an_mw_out, (size_t)n_weights_out * 4))) return rc;
    ctx->an_have_morph_targets = ctx->an_mw_have_out = false;
    if ((rc = upload(ctx, ctx->an_mw_chunks.p, chunks.data(), chunks.size() * 4))) return rc;
    if ((rc = upload(ctx, ctx->an_mw_bindings.p, bindings, (size_t)n_bindings * 4))) return rc;
    if ((rc = upload(ctx, ctx->an_mw_out.p, initial_weights ? initial_weights : zeros.data(), (size_t)n_weights_out * 4))) return rc;
    ctx->an_mw_player_graph.assign(player_graph, player_graph + n_players);
    ctx->an_mw_player_count.swap(count);
    ctx->an_mw_n_chunks = (uint32_t)n_chunks;
    ctx->an_mw_n_out = n_weights_out;
    ctx->an_mw_player_end = player_end;
    ctx->an_have_morph_targets = ctx->an_mw_have_out = true;
    return MI_OK;
}

int32_t mi_anim_frame_weights(mi_ctx* ctx, uint32_t n_players, const uint32_t* first_state, uint32_t n_states, const mi_anim_node_state* states, uint32_t flags) {
    ENTER(ctx);
    if (flags) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_weights: flags 0x%x", flags);
    if (!ctx->an_have_weight_tracks || !ctx->an_have_graphs || !ctx->an_have_morph_targets)
        return fail(ctx, MI_ERR_NOT_READY, "mi_anim_frame_weights before mi_anim_upload_weight_tracks, mi_anim_upload_graphs and mi_anim_upload_morph_targets");
    if (ctx->an_mw_player_end > n_players)
        return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_weights: a target names player %u, n_players = %u", ctx->an_mw_player_end - 1u, n_players);
    if ((n_players && !first_state) || (n_states && !states)) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_weights: NULL");
    uint32_t running = 0;  // morph targets of the players that run this frame
    for (uint32_t p = 0; p < n_players; ++p) {
        if (first_state[p] == MI_ANIM_NO_NODE) continue;
        if (p >= ctx->an_mw_player_graph.size() || ctx->an_mw_player_graph[p] == MI_ANIM_NO_NODE)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_weights: player %u has states and no graph", p);
        const uint32_t nodes = ctx->an_gr_graphs[ctx->an_mw_player_graph[p]].n_nodes;
        if ((uint64_t)first_state[p] + nodes > n_states)
            return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_frame_weights: player %u: states [%u,+%u) exceed %u", p, first_state[p], nodes, n_states);
        running += ctx->an_mw_player_count[p];
    }
    if (running == 0) return MI_OK;  // every player that has morph targets is left alone
    // ---- one word per player and 8 bytes per state, in the pinned staging block, as mi_anim_frame_graph ----
    void *st = nullptr, *d_st = nullptr;
    int32_t rc = stage_alloc(ctx, ((size_t)n_players + 2u * (size_t)n_states) * 4, &st);
    if (rc) return rc;
    memcpy(st, first_state, (size_t)n_players * 4);
    memcpy((uint32_t*)st + n_players, states, (size_t)n_states * 8);
    HIP_TRY(ctx, hipHostGetDevicePointer(&d_st, st, 0));
    AnimWeightArgs a{};
    a.n_chunks = ctx->an_mw_n_chunks;
    a.chunks = (const uint32_t*)ctx->an_mw_chunks.p;
    a.bindings = (const uint32_t*)ctx->an_mw_bindings.p;
    a.prog = (const uint32_t*)ctx->an_gr_prog.p;
    a.tracks = (const uint32_t*)ctx->an_mw_tracks.p;
    a.times = (const float*)ctx->an_mw_times.p;
    a.values = (const float*)ctx->an_mw_values.p;
    a.first_state = (const uint32_t*)d_st;
    a.states = (const uint32_t*)d_st + n_players;
    a.weights = (float*)ctx->an_mw_out.p;
    HIP_TRY(ctx, launch_anim_weights(a, ctx->stream));
    return MI_OK;
}

int32_t mi_anim_download_weights(mi_ctx* ctx, uint32_t first_weight, uint32_t n, float* out) {
    ENTER(ctx);
    if (!ctx->an_mw_have_out) return fail(ctx, MI_ERR_NOT_READY, "mi_anim_download_weights before mi_anim_upload_morph_targets");
    if ((uint64_t)first_weight + n > ctx->an_mw_n_out)
        return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_download_weights: weights [%u,+%u) exceed %u", first_weight, n, ctx->an_mw_n_out);
    if (n == 0) return MI_OK;
    if (!out) return fail(ctx, MI_ERR_INVALID_ARG, "mi_anim_download_weights: NULL");
    return download(ctx, out, (const float*)ctx->an_mw_out.p + first_weight, (size_t)n * 4);
}

}  // extern "C"
