// Training meters of engine/processor.py:97-105 (accuracy of the first score head, the two AverageMeter updates) without the
// loop's host reads, gfx950.  A tail kernel: B x num_classes floats (128 x 171 at the shipped shapes) once per iteration; its
// job is to keep the iteration free of `.item()` so that the whole step, meters included, replays from a hipGraph.
// ONE workgroup does everything: no partial counters, no ticket, nothing to reset between launches, and every sum is taken
// in a fixed order, so the state is bit-reproducible and a replay is as good as a launch.
#include <limits.h>

#include "common.h"
#include "../../include/editor_hip.h"

namespace {

constexpr int METER_THREADS = 1024;
constexpr int METER_WAVES = METER_THREADS / EDITOR_WAVE;

// is (av, ai) the row's argmax rather than (bv, bi)?  torch.max(1)[1]: a NaN beats every number, equal values (and two NaNs)
// go to the lower index.  +0 and -0 are equal.
__device__ __forceinline__ bool meter_better(float av, int ai, float bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    if (an != bn) return an;
    if (!an && av != bv) return av > bv;
    return ai < bi;
}

// one wave per row (rows w, w + 16, ...), lanes striding the columns; the wave reduction carries (value, index)
__global__ __launch_bounds__(METER_THREADS) void train_meter_kernel(const float* __restrict__ score, long lds,
    const long* __restrict__ target, const float* __restrict__ loss, int B, int C, double* __restrict__ state, int* __restrict__ last)
{
    __shared__ int hits[METER_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int mine = 0;
    for (int r = w; r < B; r += METER_WAVES) {
        const float* x = score + (long)r * lds;
        float bv = -INFINITY;
        int bi = INT_MAX;                                    // a lane without a column (C < 64) loses to every real one
        for (int c = lane; c < C; c += EDITOR_WAVE) {        // columns in rising order: only a strictly better one replaces
            const float v = x[c];
            if (bi == INT_MAX || (v != v && bv == bv) || v > bv) { bv = v; bi = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (meter_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        mine += (long)bi == target[r];                       // a target outside [0, C) never matches
    }
    if (lane == 0) hits[w] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int correct = 0;
        for (int i = 0; i < METER_WAVES; ++i) correct += hits[i];
        state[0] += (double)loss[0] * (double)B;             // loss_meter.update(loss.item(), B)
        state[1] += (double)B;
        state[2] += (double)((float)correct / (float)B);     // acc_meter.update((... == target).float().mean(), 1)
        state[3] += 1.0;
        last[0] = correct;
        last[1] = B;
    }
}

}  // namespace

extern "C" {

int editor_train_meter(const float* score, long lds, const long* target, const float* loss, int B, int C, double* state, int* last,
                       editor_stream_t stream)
{
    if (B < 1 || C < 1 || lds < C || !score || !target || !loss || !state || !last) return 1;
    train_meter_kernel<<<1, METER_THREADS, 0, (hipStream_t)stream>>>(score, lds, target, loss, B, C, state, last);
    EDITOR_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
