// Per-query top-k rank lists without the Q x G ranking (the `re.txt` lists of
// utils/metrics.py:92-99, and "the k best matches of a query" at deployment gallery sizes), gfx950.
// A filtered running selection over blocks of gallery columns: the keys are build_keys_kernel's
// (orderable distance << 32 | global gallery index, csrc/retrieval.hip), so the K smallest kept keys in ascending order
// ARE the first K kept entries of editor_rank_sort's ranking - ties by gallery index, bit-reproducible.
//   rank_topk_kernel        one workgroup per (query, slice of the block's columns): streams the row with 16-byte loads, drops
//                           keys not below the current K-th best and junk (the query's pid AND aux id), compacts the
//                           survivors with __ballot / __popcll into an LDS candidate buffer, merges a full buffer into the
//                           list with the bitonic compare-exchange network
//   rank_topk_merge_kernel  slices > 1 only: one workgroup per query folds the slices' partial lists into the running list
//   rank_topk_finish_kernel keys -> (index, distance); the distance is the inverse of `orderable`, no gather
#include "common.h"
#include "../../include/editor_hip.h"

namespace {

typedef unsigned long long u64;
constexpr int TK_THREADS = 256;
constexpr int TK_WAVES = TK_THREADS / 64;
constexpr int TK_LIST = 1024;                 // list half of the LDS buffer: K <= 1024 keys, the rest all-ones
constexpr int TK_BUF = 2 * TK_LIST;           // candidate half: filled from the top down
constexpr int TK_PER = 4;                     // keys per thread and tile (one 16-byte load)
constexpr int TK_TILE = TK_THREADS * TK_PER;  // <= TK_LIST: after a merge a whole tile's survivors fit
constexpr u64 TK_EMPTY = ~0ull;

__device__ __forceinline__ unsigned tk_orderable(float f) {          // retrieval.hip's `orderable`
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float tk_distance(unsigned h) {           // its inverse
    return __uint_as_float((h & 0x80000000u) ? (h & 0x7fffffffu) : ~h);
}

// s[0, TK_LIST): the list, ascending, all-ones past K.  s[TK_BUF - cnt, TK_BUF): cnt >= 1 candidates in any order.
// Sorts the candidates DESCENDING inside the smallest power-of-two window at the top, which makes the whole buffer bitonic
// (up, all-ones plateau, down); one half-cleaner step leaves the TK_LIST smallest in the list half, a bitonic merge orders them.
// Called by every thread of the block; ends on a barrier.
__device__ void tk_merge(u64* s, int cnt, int K)
{
    const int tid = threadIdx.x;
    int m = 2;
    while (m < cnt) m <<= 1;
    const int lo = TK_BUF - m;
    for (int e = TK_LIST + tid; e < TK_BUF - cnt; e += TK_THREADS) s[e] = TK_EMPTY;
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (m >> 1); t += TK_THREADS) {
                const int i = ((t / j) * 2 * j) + (t % j);
                const bool asc = (i & k) != 0;                      // i < m: the last stage (k = m) is descending throughout
                const u64 a = s[lo + i], b = s[lo + i + j];
                if ((a > b) == asc) { s[lo + i] = b; s[lo + i + j] = a; }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < TK_LIST; i += TK_THREADS) {
        const u64 b = s[i + TK_LIST];
        if (b < s[i]) s[i] = b;
    }
    __syncthreads();
    for (int j = TK_LIST >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (TK_LIST >> 1); t += TK_THREADS) {
            const int i = ((t / j) * 2 * j) + (t % j);
            const u64 a = s[i], b = s[i + j];
            if (a > b) { s[i] = b; s[i + j] = a; }
        }
        __syncthreads();
    }
    for (int e = K + tid; e < TK_LIST; e += TK_THREADS) s[e] = TK_EMPTY;
    __syncthreads();
}

// One tile: every thread brings TK_PER keys and their keep flags.  The tile's survivors are counted first (one barrier), so a
// buffer they would overflow is merged before they are written; `cnt` and `thr` are block-uniform registers.  wtot is
// double-buffered by `par`: a wave's next write to the same half comes after the barrier of the call in between.
__device__ __forceinline__ void tk_append(u64* s, int (*wtot)[TK_WAVES], int& par, int& cnt, u64& thr, u64 floor_key, int K,
                                          const u64 (&key)[TK_PER], const bool (&keep)[TK_PER])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    int off[TK_PER], w = 0;
#pragma unroll
    for (int j = 0; j < TK_PER; ++j) {
        const u64 b = __ballot(keep[j]);
        off[j] = w + __popcll(b & lt);
        w += __popcll(b);
    }
    if (lane == 0) wtot[par][wave] = w;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int i = 0; i < TK_WAVES; ++i) {
        const int c = wtot[par][i];
        if (i < wave) base += c;
        total += c;
    }
    par ^= 1;
    if (total == 0) return;
    if (cnt + total > TK_LIST) {
        tk_merge(s, cnt, K);
        cnt = 0;
        const u64 kth = s[K - 1];
        thr = kth < floor_key ? kth : floor_key;
    }
#pragma unroll
    for (int j = 0; j < TK_PER; ++j)
        if (keep[j]) s[TK_BUF - 1 - (cnt + base + off[j])] = key[j];
    cnt += total;
}

// grid.x = Q * slices.  slices == 1: the running list is updated in place.  slices > 1: every slice starts from an empty list,
// bounded by the running list's K-th key, and writes its K best to work[(q * slices + slice) * K].
__global__ void __launch_bounds__(TK_THREADS) rank_topk_kernel(const float* __restrict__ dist, long ldd, int Gc, long g0,
    const long* __restrict__ q_pids, const long* __restrict__ g_pids, const long* __restrict__ q_aux,
    const long* __restrict__ g_aux, int K, u64* __restrict__ list, u64* __restrict__ work, int slices)
{
    __shared__ u64 s[TK_BUF];
    __shared__ int wtot[2][TK_WAVES];
    const int tid = threadIdx.x;
    const long q = blockIdx.x / slices;
    const int sl = blockIdx.x % slices;
    const bool part = slices > 1;
    const u64* run = list + q * K;
    for (int e = tid; e < TK_LIST; e += TK_THREADS) s[e] = (!part && e < K) ? run[e] : TK_EMPTY;
    const u64 floor_key = run[K - 1];
    u64 thr = floor_key;
    __syncthreads();

    long per = ((long)Gc + slices - 1) / slices;
    per = (per + TK_PER - 1) / TK_PER * TK_PER;
    const long c0 = sl * per;
    const long c1 = c0 + per < (long)Gc ? c0 + per : (long)Gc;
    const float* row = dist + q * ldd;
    // tiles start at the 16-byte boundary at or below the slice's first column; columns below c0 are masked
    const long start = c0 - (long)(((uintptr_t)(row + c0) >> 2) & 3);
    const bool filt = q_pids != nullptr;
    const long qp = filt ? q_pids[q] : 0, qa = filt ? q_aux[q] : 0;

    int cnt = 0, par = 0;
    for (long t0 = start; t0 < c1; t0 += TK_TILE) {
        const long c = t0 + (long)tid * TK_PER;
        float v[TK_PER];
        if (c >= c0 && c + TK_PER <= c1) {
            const float4 x = *reinterpret_cast<const float4*>(row + c);
            v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
        } else {
#pragma unroll
            for (int j = 0; j < TK_PER; ++j) v[j] = (c + j >= c0 && c + j < c1) ? row[c + j] : 0.f;
        }
        u64 key[TK_PER];
        bool keep[TK_PER];
#pragma unroll
        for (int j = 0; j < TK_PER; ++j) {
            const long g = g0 + c + j;
            key[j] = ((u64)tk_orderable(v[j]) << 32) | (unsigned)g;
            keep[j] = c + j >= c0 && c + j < c1 && key[j] < thr;
            // the id arrays (16 bytes per entry against the distance's 4) are read only for keys that would enter
            if (keep[j] && filt && g_pids[g] == qp && g_aux[g] == qa) keep[j] = false;
        }
        tk_append(s, wtot, par, cnt, thr, floor_key, K, key, keep);
    }
    if (cnt) tk_merge(s, cnt, K);
    else __syncthreads();
    u64* dst = part ? work + ((long)blockIdx.x) * K : list + q * K;
    for (int e = tid; e < K; e += TK_THREADS) dst[e] = s[e];
}

// slices > 1: work[q] holds slices * K keys (each slice's list, all-ones where short); fold them into the running list
__global__ void __launch_bounds__(TK_THREADS) rank_topk_merge_kernel(const u64* __restrict__ work, int n, int K,
                                                                     u64* __restrict__ list)
{
    __shared__ u64 s[TK_BUF];
    __shared__ int wtot[2][TK_WAVES];
    const int tid = threadIdx.x;
    const long q = blockIdx.x;
    u64* run = list + q * K;
    for (int e = tid; e < TK_LIST; e += TK_THREADS) s[e] = e < K ? run[e] : TK_EMPTY;
    u64 thr = run[K - 1];
    __syncthreads();
    const u64* src = work + q * n;
    int cnt = 0, par = 0;
    for (int t0 = 0; t0 < n; t0 += TK_TILE) {
        u64 key[TK_PER];
        bool keep[TK_PER];
#pragma unroll
        for (int j = 0; j < TK_PER; ++j) {
            const int c = t0 + j * TK_THREADS + tid;
            key[j] = c < n ? src[c] : TK_EMPTY;
            keep[j] = key[j] < thr;                                // all-ones keys never pass: thr <= all-ones
        }
        tk_append(s, wtot, par, cnt, thr, TK_EMPTY, K, key, keep);
    }
    if (cnt) tk_merge(s, cnt, K);
    else __syncthreads();
    for (int e = tid; e < K; e += TK_THREADS) run[e] = s[e];
}

__global__ void rank_topk_finish_kernel(const u64* __restrict__ list, long n, int* __restrict__ index, float* __restrict__ dist)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 k = list[i];
    const bool empty = k == TK_EMPTY;
    index[i] = empty ? -1 : (int)(unsigned)(k & 0xffffffffull);
    dist[i] = empty ? __uint_as_float(0x7f800000u) : tk_distance((unsigned)(k >> 32));
}

}  // namespace

extern "C" {

int editor_rank_topk(const float* dist, long ldd, int Q, int Gc, long g0, const long* q_pids, const long* g_pids,
                     const long* q_aux, const long* g_aux, int K, unsigned long long* list, unsigned long long* work,
                     int slices, editor_stream_t stream)
{
    if (Q <= 0 || Gc <= 0 || ldd < Gc || K < 1 || K > TK_LIST) return 1;
    if (g0 < 0 || g0 + (long)Gc > 2147483647L) return 1;          // the key's low word holds the index; all-ones means empty
    const int ids = (q_pids != nullptr) + (g_pids != nullptr) + (q_aux != nullptr) + (g_aux != nullptr);
    if (ids != 0 && ids != 4) return 1;
    if (slices < 1 || slices > 1024 || (slices > 1 && !work) || (long)Q * slices > 2147483647L) return 1;
    hipStream_t st = (hipStream_t)stream;
    rank_topk_kernel<<<(unsigned)((long)Q * slices), TK_THREADS, 0, st>>>(dist, ldd, Gc, g0, q_pids, g_pids, q_aux, g_aux, K,
                                                                           list, work, slices);
    if (slices > 1) rank_topk_merge_kernel<<<(unsigned)Q, TK_THREADS, 0, st>>>(work, slices * K, K, list);
    EDITOR_LAUNCH_CHECK();
    return 0;
}

int editor_rank_topk_finish(const unsigned long long* list, int Q, int K, int* index, float* dist, editor_stream_t stream)
{
    if (Q <= 0 || K < 1 || K > TK_LIST) return 1;
    const long n = (long)Q * K;
    rank_topk_finish_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(list, n, index, dist);
    EDITOR_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
