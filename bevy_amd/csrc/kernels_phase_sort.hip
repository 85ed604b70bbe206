// kernels_phase_sort.hip -- sort_phase_system on the device: view-distance keys of one VisibleEntities list and a stable LSD radix
// sort of them (render_phase/mod.rs: sort_phase_system -> SortedPhaseItem::sort -> radsort::sort_by_key(items, |i| i.distance);
// ViewRangefinder3d::distance_translation, rangefinder.rs).  The shape of the launches is described in kernels.h.
//
// A tile is up to PS_ONE_WG_MAX = 8192 items and one workgroup of 16 waves; a tile of `count` items runs R = ceil(count / 1024)
// rounds, wave w holding items [(w R + r) 64, + 64) of round r in its registers (one 64-bit pair per lane and round): consecutive
// items belong to consecutive (wave, round, lane), which is what makes the ranking below stable.  Slots past the end of the tile hold
// the pair ~0: digit 255 in every pass and last in the tile, so they stay behind every real item and are never written out.
//
// LDS per workgroup (dynamic, 83 008 B): 8192 pairs (64 KB) | 16 histogram rows of 256 counters (16 KB) | 256 global bases | 16
// wave totals.  The pairs are NOT ping-ponged between two LDS arrays: a pass reads them from registers, and the registers are
// reloaded from the one array after the scatter -- half the LDS of the two-array form for the same traffic.
#include "glam_math.h"
#include "kernels.h"

namespace mi {
namespace {

constexpr uint32_t PS_THREADS = 1024, PS_WAVES = PS_THREADS / 64, PS_ROUNDS = PS_ONE_WG_MAX / PS_THREADS;
constexpr uint64_t PS_PAD = ~0ull;
constexpr uint32_t PS_LDS_BYTES = PS_ONE_WG_MAX * 8 + PS_WAVES * PS_DIGITS * 4 + PS_DIGITS * 4 + PS_WAVES * 4;
static_assert(PS_ROUNDS == 8 && PS_WAVES * PS_DIGITS == 4 * PS_THREADS, "the scan below takes four counters per thread");

struct PsLds {
    uint64_t* sorted;  // [PS_ONE_WG_MAX] the tile in the pass's order
    uint32_t* hist;    // [PS_WAVES][PS_DIGITS] counts of a wave's items per digit, then their exclusive offsets in the tile
    uint32_t* gbase;   // [PS_DIGITS] where the tile's run of each digit starts in the whole list (tiled form)
    uint32_t* wtot;    // [PS_WAVES]
};
__device__ __forceinline__ PsLds ps_lds() {
    extern __shared__ uint64_t ps_mem[];
    PsLds s;
    s.sorted = ps_mem;
    s.hist = reinterpret_cast<uint32_t*>(ps_mem + PS_ONE_WG_MAX);
    s.gbase = s.hist + PS_WAVES * PS_DIGITS;
    s.wtot = s.gbase + PS_DIGITS;
    return s;
}

__device__ __forceinline__ uint32_t ps_digit(uint64_t pair, uint32_t shift) { return (uint32_t)(pair >> shift) & 255u; }
__device__ __forceinline__ uint32_t ps_count_of(const PhaseSortArgs& a) { return min(*a.list_count, a.n); }
__device__ __forceinline__ const uint32_t* ps_list_of(const PhaseSortArgs& a) { return a.list + (a.list_base ? *a.list_base : 0ull); }

// distance = dot4(row2, (translation, 1)) + depth_bias, its bits mapped so that u32 order is the float order:
// -inf < negatives < -0 < +0 < positives < +inf, NaNs at either end by their sign
__device__ __forceinline__ uint64_t ps_make_pair(const PhaseSortArgs& a, uint32_t row) {
    row = min(row, a.n - 1u);
    const float* g = a.global + (size_t)row * 12u;
    const float bias = a.depth_bias ? a.depth_bias[row] : 0.0f;
    const float d = dot4(V4{a.row2[0], a.row2[1], a.row2[2], a.row2[3]}, V4{g[9], g[10], g[11], 1.0f}) + bias;
    const uint32_t bits = __float_as_uint(d);
    const uint32_t key = bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    return ((uint64_t)key << 32) | row;
}

__device__ __forceinline__ void ps_emit(const PhaseSortArgs& a, uint32_t i, uint64_t pair) {
    if (i >= a.n) return;
    const uint32_t row = (uint32_t)pair, key = (uint32_t)(pair >> 32);
    __builtin_nontemporal_store(row, a.out_rows + i);
    __builtin_nontemporal_store(a.entity_keys ? a.entity_keys[row] : (uint64_t)row, a.out_keys + i);
    __builtin_nontemporal_store(__uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu)), a.out_distance + i);  // the inverse key map
}

// The ranking primitive.  The lanes of the wave that hold the digit of this lane: eight ballots, one per digit bit, each or its
// complement ANDed in.
__device__ __forceinline__ uint64_t ps_same_digit(uint32_t digit) {
    uint64_t m = ~0ull;
#pragma unroll
    for (uint32_t b = 0; b < 8u; ++b) {
        const bool bit = (digit >> b) & 1u;
        const uint64_t bal = __builtin_amdgcn_ballot_w64(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

// Counting half: pos[r] = how many items of this wave with the same digit come before item r of this lane (earlier rounds: the
// wave's histogram row so far; this round: the lanes below), and the row ends as the wave's digit counts.  The lowest lane of each
// digit group adds the group to the row: one writer per counter, no atomics.
__device__ __forceinline__ void ps_count_tile(const PsLds& s, const uint64_t (&pair)[PS_ROUNDS], uint32_t rounds, uint32_t shift, uint32_t (&pos)[PS_ROUNDS]) {
    const uint32_t wv = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) s.hist[threadIdx.x + k * PS_THREADS] = 0u;
    __syncthreads();
    uint32_t* row = s.hist + wv * PS_DIGITS;
#pragma unroll
    for (uint32_t r = 0; r < PS_ROUNDS; ++r) {
        pos[r] = 0u;
        if (r < rounds) {  // (uniform over the workgroup)
            const uint32_t d = ps_digit(pair[r], shift);
            const uint64_t m = ps_same_digit(d);
            const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            const uint32_t before = row[d];
            pos[r] = before + below;
            MI_WAVE_LDS_SYNC();  // every lane has read the row
            if (below == 0u) row[d] = before + (uint32_t)__popcll(m);
            MI_WAVE_LDS_SYNC();
        }
    }
    __syncthreads();
}

// Scanning half: the 16 x 256 counts become exclusive offsets in (digit, wave) order -- thread t takes digit t / 4, waves
// 4 (t % 4) .. + 3, so the threads' quads are consecutive in that order -- and pos[] becomes the item's position in the sorted tile.
__device__ __forceinline__ void ps_scan_tile(const PsLds& s, const uint64_t (&pair)[PS_ROUNDS], uint32_t rounds, uint32_t shift, uint32_t (&pos)[PS_ROUNDS]) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t d = threadIdx.x >> 2, w0 = (threadIdx.x & 3u) * 4u;
    uint32_t v[4], sum = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        v[k] = s.hist[(w0 + k) * PS_DIGITS + d];
        sum += v[k];
    }
    uint32_t incl = sum;
#pragma unroll
    for (uint32_t off = 1u; off < 64u; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63u) s.wtot[wv] = incl;
    __syncthreads();
    uint32_t run = incl - sum;
#pragma unroll
    for (uint32_t k = 0; k < PS_WAVES; ++k) run += k < wv ? s.wtot[k] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        s.hist[(w0 + k) * PS_DIGITS + d] = run;
        run += v[k];
    }
    __syncthreads();
    const uint32_t* row = s.hist + wv * PS_DIGITS;
#pragma unroll
    for (uint32_t r = 0; r < PS_ROUNDS; ++r)
        if (r < rounds) pos[r] += row[ps_digit(pair[r], shift)];
}

// ---- up to PS_ONE_WG_MAX items: one workgroup, one launch ----
__global__ __launch_bounds__(PS_THREADS) void k_phase_sort_one(const PhaseSortArgs a) {
    const uint32_t count = ps_count_of(a);
    if (threadIdx.x == 0) *a.out_count = count;  // (the tiled form leaves this word to this kernel)
    if (count == 0u || count > PS_ONE_WG_MAX) return;
    const PsLds s = ps_lds();
    const uint32_t* list = ps_list_of(a);
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t rounds = (count + PS_THREADS - 1u) / PS_THREADS;
    uint64_t pair[PS_ROUNDS];
    uint32_t pos[PS_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < PS_ROUNDS; ++r) {
        const uint32_t i = (wv * rounds + r) * 64u + lane;
        pair[r] = (r < rounds && i < count) ? ps_make_pair(a, list[i]) : PS_PAD;
    }
#pragma unroll 1
    for (uint32_t shift = 32u; shift < 64u; shift += 8u) {
        ps_count_tile(s, pair, rounds, shift, pos);
        ps_scan_tile(s, pair, rounds, shift, pos);
#pragma unroll
        for (uint32_t r = 0; r < PS_ROUNDS; ++r)
            if (r < rounds) s.sorted[pos[r]] = pair[r];
        __syncthreads();
        if (shift < 56u) {
#pragma unroll
            for (uint32_t r = 0; r < PS_ROUNDS; ++r)
                if (r < rounds) pair[r] = s.sorted[(wv * rounds + r) * 64u + lane];
        }
    }
    for (uint32_t i = threadIdx.x; i < count; i += PS_THREADS) ps_emit(a, i, s.sorted[i]);
}

// ---- longer lists: tiles of PS_ONE_WG_MAX items ----
__global__ __launch_bounds__(PS_THREADS) void k_phase_keys(const PhaseSortArgs a) {
    const uint32_t count = ps_count_of(a);
    if (count <= PS_ONE_WG_MAX) return;
    const uint32_t i = blockIdx.x * PS_THREADS + threadIdx.x;
    if (i < count) __builtin_nontemporal_store(ps_make_pair(a, ps_list_of(a)[i]), a.pairs[0] + i);
}

// What a tile workgroup of the tiled form starts with: its items in registers; false = nothing to do
__device__ __forceinline__ bool ps_load_tile(const PhaseSortArgs& a, const uint64_t* src, uint64_t (&pair)[PS_ROUNDS], uint32_t* tile_count, uint32_t* rounds,
                                             uint32_t* n_tiles) {
    const uint32_t count = ps_count_of(a);
    const uint32_t base = blockIdx.x * PS_ONE_WG_MAX;
    if (count <= PS_ONE_WG_MAX || base >= count) return false;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    *n_tiles = (count + PS_ONE_WG_MAX - 1u) / PS_ONE_WG_MAX;
    *tile_count = min(count - base, PS_ONE_WG_MAX);
    *rounds = (*tile_count + PS_THREADS - 1u) / PS_THREADS;
#pragma unroll
    for (uint32_t r = 0; r < PS_ROUNDS; ++r) {
        const uint32_t i = (wv * *rounds + r) * 64u + lane;
        pair[r] = (r < *rounds && i < *tile_count) ? src[base + i] : PS_PAD;
    }
    return true;
}

// 1. the tile's digit counts into the digit-major table [256][tiles]
__global__ __launch_bounds__(PS_THREADS) void k_ps_hist(const PhaseSortArgs a, const uint64_t* src, uint32_t shift) {
    uint64_t pair[PS_ROUNDS];
    uint32_t pos[PS_ROUNDS], tile_count, rounds, n_tiles;
    if (!ps_load_tile(a, src, pair, &tile_count, &rounds, &n_tiles)) return;
    const PsLds s = ps_lds();
    ps_count_tile(s, pair, rounds, shift, pos);
    if (threadIdx.x < PS_DIGITS) {
        uint32_t c = 0u;
#pragma unroll
        for (uint32_t w = 0; w < PS_WAVES; ++w) c += s.hist[w * PS_DIGITS + threadIdx.x];
        if (threadIdx.x == 255u) c -= rounds * PS_THREADS - tile_count;  // the padding
        a.table[threadIdx.x * n_tiles + blockIdx.x] = c;
    }
}

// 2. one workgroup: the exclusive scan of the table in (digit, tile) order, 16 consecutive counters per thread and round (four
// 16-byte loads in flight per lane: the table is 256 x tiles words, a whole number of quads)
__global__ __launch_bounds__(PS_THREADS) void k_ps_scan(const PhaseSortArgs a) {
    const uint32_t count = ps_count_of(a);
    if (count <= PS_ONE_WG_MAX) return;
    const uint32_t total = PS_DIGITS * ((count + PS_ONE_WG_MAX - 1u) / PS_ONE_WG_MAX);
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    __shared__ uint32_t wtot[PS_WAVES];
    uint4* const table4 = reinterpret_cast<uint4*>(a.table);
    uint32_t carry = 0u;
    for (uint32_t base = 0; base < total; base += 16u * PS_THREADS) {
        const uint32_t i0 = base + threadIdx.x * 16u;
        uint4 q[4];
        uint32_t sum = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            q[k] = i0 + 4u * k < total ? table4[(i0 >> 2) + k] : uint4{0u, 0u, 0u, 0u};
            sum += (q[k].x + q[k].y) + (q[k].z + q[k].w);
        }
        uint32_t incl = sum;
#pragma unroll
        for (uint32_t off = 1u; off < 64u; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63u) wtot[wv] = incl;
        __syncthreads();
        uint32_t run = carry + incl - sum, all = 0u;
#pragma unroll
        for (uint32_t k = 0; k < PS_WAVES; ++k) {
            run += k < wv ? wtot[k] : 0u;
            all += wtot[k];
        }
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint4 e{run, run + q[k].x, run + q[k].x + q[k].y, run + q[k].x + q[k].y + q[k].z};
            run = e.w + q[k].w;
            if (i0 + 4u * k < total) table4[(i0 >> 2) + k] = e;
        }
        carry += all;
        __syncthreads();  // wtot is rewritten by the next round
    }
}

// 3. the scatter: the tile is ranked again, ordered by digit in LDS, and each digit's run leaves as one contiguous store at its
// scanned offset.  LAST: the pass over the top digit writes rows / entity keys / distances instead of pairs.
template <bool LAST>
__global__ __launch_bounds__(PS_THREADS) void k_ps_scatter(const PhaseSortArgs a, const uint64_t* src, uint64_t* dst, uint32_t shift) {
    uint64_t pair[PS_ROUNDS];
    uint32_t pos[PS_ROUNDS], tile_count, rounds, n_tiles;
    if (!ps_load_tile(a, src, pair, &tile_count, &rounds, &n_tiles)) return;
    const PsLds s = ps_lds();
    if (threadIdx.x < PS_DIGITS) s.gbase[threadIdx.x] = a.table[threadIdx.x * n_tiles + blockIdx.x];
    ps_count_tile(s, pair, rounds, shift, pos);
    ps_scan_tile(s, pair, rounds, shift, pos);
#pragma unroll
    for (uint32_t r = 0; r < PS_ROUNDS; ++r)
        if (r < rounds) s.sorted[pos[r]] = pair[r];
    __syncthreads();
    for (uint32_t p = threadIdx.x; p < tile_count; p += PS_THREADS) {
        const uint64_t pr = s.sorted[p];
        const uint32_t d = ps_digit(pr, shift);
        const uint32_t i = s.gbase[d] + (p - s.hist[d]);  // (hist[d] = wave 0's offset = where the digit's run starts in the tile)
        if (LAST) ps_emit(a, i, pr);
        else if (i < a.n) dst[i] = pr;
    }
}

}  // namespace

hipError_t set_phase_sort_lds_limit() {
    const void* fns[] = {reinterpret_cast<const void*>(k_phase_sort_one), reinterpret_cast<const void*>(k_ps_hist),
                         reinterpret_cast<const void*>(k_ps_scatter<false>), reinterpret_cast<const void*>(k_ps_scatter<true>)};
    for (const void* f : fns) {
        hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PS_LDS_BYTES);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_phase_sort(const PhaseSortArgs& a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    MI_LAUNCH(k_phase_sort_one, dim3(1), dim3(PS_THREADS), PS_LDS_BYTES, stream, a);
    if (a.n > PS_ONE_WG_MAX) {
        const uint32_t tiles = (a.n + PS_ONE_WG_MAX - 1u) / PS_ONE_WG_MAX;
        MI_LAUNCH(k_phase_keys, dim3((a.n + PS_THREADS - 1u) / PS_THREADS), dim3(PS_THREADS), 0, stream, a);
        for (uint32_t pass = 0; pass < 4u; ++pass) {
            const uint64_t* src = a.pairs[pass & 1u];
            uint64_t* dst = a.pairs[(pass & 1u) ^ 1u];
            const uint32_t shift = 32u + 8u * pass;
            MI_LAUNCH(k_ps_hist, dim3(tiles), dim3(PS_THREADS), PS_LDS_BYTES, stream, a, src, shift);
            MI_LAUNCH(k_ps_scan, dim3(1), dim3(PS_THREADS), 0, stream, a);
            if (pass < 3u) MI_LAUNCH(k_ps_scatter<false>, dim3(tiles), dim3(PS_THREADS), PS_LDS_BYTES, stream, a, src, dst, shift);
            else MI_LAUNCH(k_ps_scatter<true>, dim3(tiles), dim3(PS_THREADS), PS_LDS_BYTES, stream, a, src, dst, shift);
        }
    }
    return hipGetLastError();
}

}  // namespace mi
