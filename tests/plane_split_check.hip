// Stand-alone device check of csrc/plane_split.h (tests/test_gpu_plane_split.py builds and runs it): irs_split2h against the
// plain statement h = (_Float16)v, l = (_Float16)(v - (float)h), bit for bit, over EVERY float32 pattern -- which holds every
// exponent from the subnormals up with all its mantissas, both zeros, the 2^16 exact float16 values, the whole range where l
// is a float16 subnormal, and everything up to and beyond 32752 -- each pattern once in each half of the pair.
// One line of output: "plane_split_check patterns=N slots=2 finite_diff=A nonfinite_bad=B first=<hex,..>"; exit status 0 iff A = B = 0.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "plane_split.h"

struct Report {
    unsigned long long finite_diff, nonfinite_bad;
    unsigned int first[8];
};

__device__ __forceinline__ bool f16_nan(unsigned int b) { return (b & 0x7FFFu) > 0x7C00u; }

// one value's planes: equal bits, or (input not finite only) both NaN
__device__ void judge(unsigned int u, unsigned int h, unsigned int l, unsigned int rh, unsigned int rl, Report *rep) {
    if (h == rh && l == rl) return;
    const bool finite = (u & 0x7F800000u) != 0x7F800000u;
    if (!finite && (h == rh || (f16_nan(h) && f16_nan(rh))) && (l == rl || (f16_nan(l) && f16_nan(rl)))) return;
    const unsigned long long k = atomicAdd(finite ? &rep->finite_diff : &rep->nonfinite_bad, 1ull);
    if (finite && k < 8) rep->first[k] = u;
}

__global__ void __launch_bounds__(256) k_check(Report *rep) {
    const unsigned int base = (blockIdx.x * 256u + threadIdx.x) << 8; // 2^16 blocks x 256 threads x 256 patterns = 2^32
    for (unsigned int i = 0; i < 256u; ++i) {
        const unsigned int u0 = base + i, u1 = u0 * 2654435761u + 0x9E3779B9u; // (odd multiplier: u1 runs over every pattern too)
        const float v0 = __uint_as_float(u0), v1 = __uint_as_float(u1);
        irs_f16x2 hp, lp, rh, rl;
        irs_split2h(v0, v1, hp, lp);
        irs_split2h_plain(v0, v1, rh, rl);
        const unsigned int h = __builtin_bit_cast(unsigned int, hp), l = __builtin_bit_cast(unsigned int, lp);
        const unsigned int qh = __builtin_bit_cast(unsigned int, rh), ql = __builtin_bit_cast(unsigned int, rl);
        judge(u0, h & 0xFFFFu, l & 0xFFFFu, qh & 0xFFFFu, ql & 0xFFFFu, rep);
        judge(u1, h >> 16, l >> 16, qh >> 16, ql >> 16, rep);
    }
}

int main() {
    Report *d = nullptr, r;
    if (hipMalloc(&d, sizeof(Report)) != hipSuccess || hipMemset(d, 0, sizeof(Report)) != hipSuccess) {
        printf("plane_split_check error=no-device\n");
        return 2;
    }
    k_check<<<1u << 16, 256>>>(d);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&r, d, sizeof(Report), hipMemcpyDeviceToHost) != hipSuccess) {
        printf("plane_split_check error=%s\n", hipGetErrorString(hipGetLastError()));
        return 2;
    }
    printf("plane_split_check patterns=%llu slots=2 finite_diff=%llu nonfinite_bad=%llu first=", 1ull << 32, r.finite_diff, r.nonfinite_bad);
    for (int i = 0; i < 8 && (unsigned long long)i < r.finite_diff; ++i) printf("%s%08x", i ? "," : "", r.first[i]);
    printf("\n");
    (void)hipFree(d);
    return (r.finite_diff || r.nonfinite_bad) ? 1 : 0;
}
