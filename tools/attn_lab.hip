// Development lab for the throughput attention kernel (not product code): k_attn16<16, FAST, PLANES> on synthetic packed sequences
// with in-kernel s_memtime stamps (-DATTN_STAMP): how a workgroup's life splits into issuing the K / V loads, waiting for
// them + staging them into LDS, the barrier, and the query blocks.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -DIRS_LAB -DATTN_STAMP tools/attn_lab.hip -o tools/attn_lab ; run: tools/attn_lab [sequences=4096]
#include <cmath>
#include <cstdlib>
#include <vector>

#include "../influentialrs_amd/csrc/decoder.hip"
void irs_prof_begin(irs_ctx *, int, hipStream_t) {}
void irs_prof_end(irs_ctx *, int, hipStream_t, double, double) {}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s -> %s\n", #x, hipGetErrorString(e_)); exit(1);} } while (0)

// K and V sections of q | k | v rows -> float16 plane pairs per (token, head) (what k_block_x6's tail writes with kv_planes)
__global__ void k_lab_to_planes(const float *in, float *outp, long long rows, int d) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; // one (row, section, head, channel)
    if (i >= rows * 2 * d) return;
    const long long row = i / (2 * d);
    const int rem = (int)(i % (2 * d)), sec = rem / d, c = rem % d, head = c / 32, ch = c % 32;
    if (sec == 0) return; // (K stays float32: the scores run on the exact chain)
    const float v = in[row * 3 * d + (1 + sec) * d + c];
    const _Float16 h = (_Float16)v, l = (_Float16)(v - (float)h);
    _Float16 *slot = reinterpret_cast<_Float16 *>(outp + row * 3 * d + (1 + sec) * d + head * 32);
    slot[ch] = h;
    slot[32 + ch] = l;
}

int main(int argc, char **argv) {
    setvbuf(stdout, nullptr, _IONBF, 0);
    const int B = argc > 1 ? atoi(argv[1]) : 4096, L = 200, d = 128, H = 4;
    const int lens[8] = {40, 70, 95, 110, 130, 95, 200, 180}; // mean 115: the bench's packed windows average 109-117
    std::vector<int32_t> off(B), cnt(B), padq(B, -1);
    long long M = 0;
    const int fixed_len = argc > 3 ? atoi(argv[3]) : 0; // > 0: every sequence has this many tokens
    for (int b = 0; b < B; ++b) { off[b] = (int32_t)M; cnt[b] = fixed_len > 0 ? fixed_len : lens[(b * 5 + b / 8) & 7]; M += cnt[b]; }
    std::vector<float> hq((size_t)M * 3 * d);
    unsigned long long z = 88172645463325252ull;
    for (auto &v : hq) { z ^= z << 13; z ^= z >> 7; z ^= z << 17; v = ((float)((z >> 40) & 0xFFFFFF) * (1.0f / 16777216.0f) * 2 - 1) * 0.7f; }
    std::vector<int64_t> hseq((size_t)B * L, 1);
    float *qkv, *ru;
    int64_t *seq;
    int32_t *doff, *dcnt, *dpadq;
    CK(hipMalloc(&qkv, hq.size() * 4)); CK(hipMemcpy(qkv, hq.data(), hq.size() * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&ru, B * 4)); CK(hipMemset(ru, 0, B * 4));
    CK(hipMalloc(&seq, hseq.size() * 8)); CK(hipMemcpy(seq, hseq.data(), hseq.size() * 8, hipMemcpyHostToDevice));
    CK(hipMalloc(&doff, B * 4)); CK(hipMemcpy(doff, off.data(), B * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&dcnt, B * 4)); CK(hipMemcpy(dcnt, cnt.data(), B * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&dpadq, B * 4)); CK(hipMemcpy(dpadq, padq.data(), B * 4, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    // (the register-staged fill with the transposed V^T image, timed here against the LDS-DMA fill in round 3 --
    // profiles/r03/attn16_lab_stamps.txt -- left the tree with the kernel's template arm)
    const size_t lds16d = (size_t)2 * ((L + 15) & ~15) * 32 * 4 + 64;
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_attn16<16, true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds16d));
    float *out2;
    CK(hipMalloc(&out2, ((size_t)M + 128) * d * 4)); CK(hipMemset(out2, 0, ((size_t)M + 128) * d * 4));
    // (the persistent work-list form measured here in round 4 -- profiles/r04/attn_lab_persist_r04.txt -- left the tree in round 5)
    const int variant = argc > 2 ? atoi(argv[2]) : 1; // 1: the float32 form, 4: float32 against float16 planes
    auto timed = [&](const char *name, auto launch) {
        float ms;
        CK(hipEventRecord(e0));
        launch();
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
        CK(hipEventElapsedTime(&ms, e0, e1));
        printf("%-44s %d sequences x %d heads, %lld packed rows: %8.1f us\n", name, B, H, M, ms * 1e3);
    };
    for (int rep = 0; rep < 5; ++rep) {
        if (variant != 4)
            timed("k_attn16<16, FAST> float32:", [&] { hipLaunchKernelGGL((k_attn16<16, true, false>), dim3(H, B), dim3(256), lds16d, 0, qkv, seq, ru, out2, L, d, IRS_MASK_IRN, doff, dcnt, dpadq, 1, H); });
    }
    if (variant == 4) { // the split-float16 attention on plane-format K / V against the float32 kernel on the same values
        float *qkvp, *out4;
        CK(hipMalloc(&qkvp, hq.size() * 4)); CK(hipMemcpy(qkvp, qkv, hq.size() * 4, hipMemcpyDeviceToDevice));
        CK(hipMalloc(&out4, ((size_t)M + 128) * d * 4)); CK(hipMemset(out4, 0, ((size_t)M + 128) * d * 4));
        hipLaunchKernelGGL(k_lab_to_planes, dim3((unsigned)((M * 2 * d + 255) / 256)), dim3(256), 0, 0, qkv, qkvp, M, d);
        for (int rep = 0; rep < 3; ++rep) {
            timed("k_attn16<16, FAST> float32:", [&] { hipLaunchKernelGGL((k_attn16<16, true, false>), dim3(H, B), dim3(256), lds16d, 0, qkv, seq, ru, out2, L, d, IRS_MASK_IRN, doff, dcnt, dpadq, 1, H); });
            timed("k_attn16<16, FAST, PLANES> float16 planes:", [&] { hipLaunchKernelGGL((k_attn16<16, true, true>), dim3(H, B), dim3(256), lds16d, 0, qkvp, seq, ru, out4, L, d, IRS_MASK_IRN, doff, dcnt, dpadq, 1, attn_grid_heads{}); });
        }
        std::vector<float> h1((size_t)M * d), h2((size_t)M * d);
        CK(hipMemcpy(h1.data(), out2, h1.size() * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(h2.data(), out4, h2.size() * 4, hipMemcpyDeviceToHost));
        double md = 0, sum = 0; size_t worst = 0, n4 = 0;
        for (size_t i = 0; i < h1.size(); ++i) { const double e = fabs((double)h1[i] - h2[i]); sum += e; if (e > md) md = e, worst = i; if (e > 1e-4) ++n4; }
        // fragment-major output: float4 index ((tile * H + head) * 4 + g) * 64 + lane -> token = tile * 32 + (lane & 31)
        const size_t f4 = worst / 4, lane_ = f4 % 64, tile_ = f4 / (64 * 4 * H), head_ = (f4 / (64 * 4)) % H;
        const long long tok = (long long)tile_ * 32 + (lane_ & 31);
        int sb = 0; while (sb + 1 < B && off[sb + 1] <= tok) ++sb;
        printf("split-float16 vs float32 attention: max %.3g  mean %.3g  values > 1e-4: %zu; worst at token %lld = sequence %d (length %d) position %lld head %zu: %g vs %g\n",
               md, sum / h1.size(), n4, tok, sb, cnt[sb], tok - off[sb], head_, h2[worst], h1[worst]);
    }
#ifdef ATTN_STAMP
    {
        const size_t nw = (size_t)B * H * 4 < 65536 ? (size_t)B * H * 4 : 65536;
        std::vector<unsigned long long> hs(nw * 8);
        CK(hipMemcpyFromSymbol(hs.data(), HIP_SYMBOL(g_attn_stamp), nw * 64));
        double t[5] = {0, 0, 0, 0, 0};
        size_t n = 0;
        for (size_t w = 0; w < nw; ++w) {
            const unsigned long long *s = &hs[w * 8];
            if (!s[0] || !s[4] || s[4] < s[0]) continue;
            t[0] += (double)(s[1] - s[0]), t[1] += (double)(s[2] - s[1]), t[2] += (double)(s[3] - s[2]), t[3] += (double)(s[4] - s[3]), t[4] += (double)(s[4] - s[0]);
            ++n;
        }
        printf("stamps (s_memtime ticks per wave, mean over %zu waves): life %.0f = issue K/V loads %.0f + wait for them, masks, stage into LDS %.0f + "
               "barrier %.0f + query blocks %.0f\n", n, t[4] / n, t[0] / n, t[1] / n, t[2] / n, t[3] / n);
    }
#endif
    return 0;
}
