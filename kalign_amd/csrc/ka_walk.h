// ka_walk.h -- the wave-per-item walk of the stages' kernels (gfx950, wave64; ka_in.hip, ka_cod.hip, ka_sum.hip, ka_out.hip).
// A wave takes one sequence or row and walks its bytes KA_WALK_STEP a step as four ballots of 64, lane l of ballot q the
// byte c0 + 64 q + l: a byte per lane, so that a row may start at any byte, and the loads of all four go out before the
// first ballot.  A lane at or past the end loads nothing and holds -1: the byte after a row, the next row and the end of the
// upload are never read.  A kept byte's place is the count carried so far plus the population count of the lower lanes of its
// ballot (ka_lanes_below).  Everything after the ballots is wave-uniform arithmetic on 64-bit masks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define KA_WALK_STEP 256           // bytes per step; a stage's own name for it (KA_IN_STEP, KA_SUM_CHUNK, KA_OUT_STEP) is this number

// the bytes of one step of n bytes at p, -1 at and past the end.  Index: the type a stage counts its bytes in
template <int STEP, typename Index>
__device__ __forceinline__ void ka_walk_step(const uint8_t* p, Index n, Index c0, int lane, int* b)
{
        static_assert(STEP == KA_WALK_STEP, "the walk is written for four ballots of 64 a step");
#pragma unroll
        for (int q = 0; q < STEP / 64; q++) {
                const Index c = c0 + 64 * q + lane;
                b[q] = c < n ? (int)p[c] : -1;
        }
}

// the lanes of a ballot below this one
__device__ __forceinline__ unsigned long long ka_lanes_below(int lane) { return (1ull << lane) - 1ull; }

// the sum over the wave's lanes, in every lane
__device__ __forceinline__ long long ka_wave_sum(long long v)
{
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
        return v;
}

// a wave per item: the workgroups of `threads` threads that n items take
inline unsigned ka_wave_grid(long long n, int threads)
{
        const int waves = threads / 64;
        return (unsigned)((n + waves - 1) / waves);
}

// A workgroup's items are consecutive, so those of one family are neighbours: thread `slot` adds up vals[w][slot] over the
// waves w of a family (famOf[w], -1: the wave has no item; written before the barrier that precedes this) and sends the sum
// with one 64-bit atomic per family the workgroup meets -- it may hold the end of one family and the start of the next -- to
// dst[family * stride + slot].  Integer sums in any order: the result does not depend on scheduling.
template <typename T, int kWaves, int kSlots>
__device__ __forceinline__ void ka_fold_families(const T (&vals)[kWaves][kSlots], const int (&famOf)[kWaves], int slot, unsigned long long* dst, int stride)
{
        unsigned long long acc = 0;
        for (int w = 0; w < kWaves && famOf[w] >= 0; w++) {
                acc += (unsigned long long)vals[w][slot];
                if (w + 1 < kWaves && famOf[w + 1] == famOf[w]) continue;
                if (acc) atomicAdd(&dst[(long long)famOf[w] * stride + slot], acc);
                acc = 0;
        }
}
