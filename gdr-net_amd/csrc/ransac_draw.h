// The counter-based draw the RANSAC kernels (pnp.hip, rigid.hip) take their minimal samples from: no RNG state, the same (seed, RoI, hypothesis, draw)
// gives the same index whatever the launch shape.  Host and device: the header of the C-ABI states the rule, the tests restate it in numpy.
#pragma once

#define PNP_HD __host__ __device__ __forceinline__

namespace {

constexpr int PNP_MAX_DRAWS = 64;     // draws a hypothesis may spend on its distinct indices before it counts as degenerate

PNP_HD unsigned long long pnp_mix64(unsigned long long x) {   // splitmix64 finaliser
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// draw `d` of hypothesis h of RoI n: an index below count.  No state: a function of (seed, n, h, d) alone.
PNP_HD int pnp_draw(unsigned long long seed, int n, int h, int d, int count) {
    const unsigned long long key = seed * 0x9E3779B97F4A7C15ull + (unsigned long long)n * 0xBF58476D1CE4E5B9ull +
                                   (unsigned long long)h * 0x94D049BB133111EBull + (unsigned long long)d * 0xD6E8FEB86659FD93ull;
    return (int)(((pnp_mix64(key) >> 32) * (unsigned long long)count) >> 32);
}

// K distinct indices below count (count >= K): a collision advances the draw counter
template <int K>
PNP_HD bool pnp_sample(unsigned long long seed, int n, int h, int count, int* idx) {
    int d = 0;
    for (int k = 0; k < K; ++k) {
        bool found = false;
        while (!found && d < PNP_MAX_DRAWS) {
            const int c = pnp_draw(seed, n, h, d++, count);
            found = true;
            for (int j = 0; j < k; ++j) found = found && (idx[j] != c);
            if (found) idx[k] = c;
        }
        if (!found) return false;
    }
    return true;
}

}  // namespace
