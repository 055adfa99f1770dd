// Float16 plane split of a float32 pair: h = f16(v), l = f16(v - float(h)), both rounded to nearest even -- the operand form
// of every 16-bit MFMA under IRS_GEMM_H3 (x, y, the FFN hidden units, the attention output, K, V, q and the probabilities).
//
// Written as `h = (_Float16)v; l = (_Float16)(v - (float)h)` the compiler converts h twice (singly to feed the conversion
// back, packed for the operand), converts each h back, SLP-packs the differences into v_pk_add_f32 and packs them again:
// 23 vector instructions per 8 values.  gfx950's mixed fma reads a float16 half of a register as a float32 source and rounds
// its float32 result to float16 into one half of the destination, so l is ONE instruction per value, reading h where the
// packed conversion left it: 3 instructions per pair.  fma(h, -1, v) = v - h is exact in float32 (h is v's nearest float16,
// or both are far below float16's range), so there is one rounding either way and the bits are those of the plain statement
// for every finite v (tests/plane_split_check.hip compares them on the device); v beyond float16's range gives h = +-inf and
// l = -+inf in both forms.
//
// The compiler does not select this by itself: fma(h, -1, v) is folded to a subtraction before instruction selection.  The
// statement is not volatile and has no memory clobber: the scheduler places it like any other arithmetic.  The outputs are
// early-clobber because h is written before v1 is read and l before its second half is computed.
//
// Where the helper does NOT apply as it stands (both found as differing bytes of the decoder's rows, profiles/plane_split):
//   * v = fma(a, b, c) with h = (_Float16)v: the compiler selects ONE mixed fma for h, which rounds the exact a b + c to
//     float16 once (measured: 6e-5 of random triples differ from f16(f32(fma))).  The K / V epilogues are such sites: they keep
//     that statement for h and take only l from here (irs_split_low).
//   * v = a * b: -ffp-contract contracts the product into the subtraction, l = f16(fma(a, b, -h)) with the product
//     unrounded.  The sequence-resident block's q is such a site and keeps the plain statement (8 values per block).
#pragma once

typedef __attribute__((ext_vector_type(2))) _Float16 irs_f16x2;

__device__ __forceinline__ void irs_split2h(float v0, float v1, irs_f16x2 &hp, irs_f16x2 &lp) {
    asm("v_cvt_pk_f16_f32 %0, %2, %3\n\t"
        "v_fma_mixlo_f16 %1, %0, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %1, %0, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
        : "=&v"(hp), "=&v"(lp)
        : "v"(v0), "v"(v1));
}

// l alone, for a pair whose h the caller holds already (where h = f16(fma(..)) is one instruction the compiler selects itself)
__device__ __forceinline__ irs_f16x2 irs_split2l(irs_f16x2 hp, float v0, float v1) {
    irs_f16x2 lp;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
        : "=&v"(lp)
        : "v"(hp), "v"(v0), "v"(v1));
    return lp;
}

// the plain statement (what the helper replaces; the reference of the device check)
__device__ __forceinline__ void irs_split2h_plain(float v0, float v1, irs_f16x2 &hp, irs_f16x2 &lp) {
    const _Float16 h0 = (_Float16)v0, h1 = (_Float16)v1;
    hp = irs_f16x2{h0, h1};
    lp = irs_f16x2{(_Float16)(v0 - (float)h0), (_Float16)(v1 - (float)h1)};
}

// N values whose h plane the caller computed (H[j] = f16 of the expression v[j] was rounded from): the l plane alone
template <int N, class V16>
__device__ __forceinline__ void irs_split_low(const float (&v)[N], const V16 &H, V16 &Lo) {
    static_assert(N % 2 == 0, "pairs");
#pragma unroll
    for (int j = 0; j < N; j += 2) {
        const irs_f16x2 lp = irs_split2l(irs_f16x2{H[j], H[j + 1]}, v[j], v[j + 1]);
        Lo[j] = lp[0], Lo[j + 1] = lp[1];
    }
}

// N values (N even) into two vectors of N float16: P[0] = h, P[1] = l
template <int N, class V16>
__device__ __forceinline__ void irs_split_planes(const float (&v)[N], V16 &H, V16 &Lo) {
    static_assert(N % 2 == 0, "pairs");
#pragma unroll
    for (int j = 0; j < N; j += 2) {
        irs_f16x2 hp, lp;
        irs_split2h(v[j], v[j + 1], hp, lp);
        H[j] = hp[0], H[j + 1] = hp[1];
        Lo[j] = lp[0], Lo[j + 1] = lp[1];
    }
}
