// Lab: which waves of a 512-thread workgroup share a SIMD.  One workgroup per CU (152 KB of LDS, like the sequence-resident
// decoder's), every wave reads its hardware id register (gfx9 HW_ID: bits 5:4 = SIMD, 11:8 = CU, 12 = SH, 15:13 = SE).
// Prints, per wave index, how many workgroups had it on SIMD 0 .. 3, and how many workgroups had waves w and w + 4 together.
// build: hipcc --offload-arch=gfx950 -O2 tools/simd_probe.hip -o tools/simd_probe_lab
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
__global__ void __launch_bounds__(512, 1) k_probe(unsigned *out) {
    extern __shared__ char smem[];
    if (threadIdx.x == 0) smem[0] = 1; // (the LDS is really allocated)
    unsigned id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(id));
    if ((threadIdx.x & 63) == 0) out[blockIdx.x * 8 + (threadIdx.x >> 6)] = id;
}
int main() {
    const int nwg = 1024, lds = 152 * 1024;
    unsigned *d;
    if (hipMalloc(&d, nwg * 8 * 4) != hipSuccess) return 1;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_probe), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(k_probe, dim3(nwg), dim3(512), lds, 0, d);
    if (hipDeviceSynchronize() != hipSuccess) return 2;
    std::vector<unsigned> h(nwg * 8);
    (void)hipMemcpy(h.data(), d, nwg * 8 * 4, hipMemcpyDeviceToHost);
    int hist[8][4] = {}, pair_same = 0, low_distinct = 0, high_distinct = 0;
    for (int w = 0; w < nwg; ++w) {
        int s[8];
        for (int k = 0; k < 8; ++k) s[k] = (h[w * 8 + k] >> 4) & 3, ++hist[k][s[k]];
        bool ps = true;
        for (int k = 0; k < 4; ++k) ps = ps && s[k] == s[k + 4];
        pair_same += ps;
        low_distinct += ((1 << s[0]) | (1 << s[1]) | (1 << s[2]) | (1 << s[3])) == 15;
        high_distinct += ((1 << s[4]) | (1 << s[5]) | (1 << s[6]) | (1 << s[7])) == 15;
    }
    for (int k = 0; k < 8; ++k) printf("wave %d: SIMD 0..3 = %d %d %d %d\n", k, hist[k][0], hist[k][1], hist[k][2], hist[k][3]);
    printf("%d workgroups: waves w and w + 4 on one SIMD in %d, waves 0..3 on four SIMDs in %d, waves 4..7 on four SIMDs in %d\n", nwg,
           pair_same, low_distinct, high_distinct);
    return 0;
}
