// philox.h -- the counter-based random stream of the EmptyDrops simulation (emptydrops.h) and of the read subsampling
// (subsample.h).  Word q of stream s is word q & 3 of Philox4x64-10(counter = (1 + (q >> 2), s, 0, 0), key = (seed, 0)):
// element q of np.random.Philox(counter=[0, s, 0, 0], key=[seed, 0]).random_raw() (numpy advances the counter before it
// generates the first block).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void cr_philox4x64_10(unsigned long long c0, unsigned long long c1, unsigned long long k0, unsigned long long w[4]) {
    unsigned long long c2 = 0, c3 = 0, k1 = 0;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long hi0 = __umul64hi(0xD2E7470EE14C6C93ull, c0), lo0 = 0xD2E7470EE14C6C93ull * c0;
        const unsigned long long hi1 = __umul64hi(0xCA5A826395121157ull, c2), lo1 = 0xCA5A826395121157ull * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B97F4A7C15ull;
        k1 += 0xBB67AE8584CAA73Bull;
    }
    w[0] = c0;
    w[1] = c1;
    w[2] = c2;
    w[3] = c3;
}
