// The screen's k-step (ONE v_mfma_f32_32x32x16_f16 + ONE ds_read_b128, one wave per SIMD) with packed-fp16 and fp16-transcendental
// fillers in EVERY MFMA gap, against the fp32 forms the screen's epilogue uses today; prints cycles per MFMA.
// Sibling of mfma_gap_fill.hip (that one is the h2 pattern: 3 MFMAs + 2 ds_read_b128 per k-step).
//   hipcc --offload-arch=gfx950 -O3 tools/micro/mfma_gap_fill_f16.hip -o tools/micro/mfma_gap_fill_f16
#include <hip/hip_runtime.h>
#include <stdio.h>

// fp32 fillers of the current epilogue (epi1_op)
#define FMA1 "v_fma_f32 v60, v60, v61, v62\n"
#define FMA2 FMA1 "v_fma_f32 v63, v63, v61, v62\n"
#define FMA3 FMA2 "v_fma_f32 v64, v64, v61, v62\n"
#define FMA4 FMA3 "v_fma_f32 v65, v65, v61, v62\n"
#define FMA5 FMA4 "v_fma_f32 v66, v66, v61, v62\n"
#define EXP1 "v_exp_f32 v68, v68\n"
#define EXP2 EXP1 "v_log_f32 v69, v69\n"
// packed fp16
#define PKM1 "v_pk_mul_f16 v72, v72, v61\n"
#define PKM2 PKM1 "v_pk_mul_f16 v73, v73, v61\n"
#define PKM3 PKM2 "v_pk_mul_f16 v74, v74, v61\n"
#define PKM4 PKM3 "v_pk_mul_f16 v75, v75, v61\n"
#define PKA1 "v_pk_add_f16 v72, v72, v61\n"
#define PKA2 PKA1 "v_pk_add_f16 v73, v73, v61\n"
#define PKA3 PKA2 "v_pk_add_f16 v74, v74, v61\n"
#define PKF1 "v_pk_fma_f16 v72, v72, v61, v62\n"
#define PKF2 PKF1 "v_pk_fma_f16 v73, v73, v61, v62\n"
#define PKF3 PKF2 "v_pk_fma_f16 v74, v74, v61, v62\n"
#define PKF4 PKF3 "v_pk_fma_f16 v75, v75, v61, v62\n"
#define PKX1 "v_pk_max_f16 v72, v72, v61\n"
#define PKX2 PKX1 "v_pk_max_f16 v73, v73, v61\n"
#define PKX3 PKX2 "v_pk_max_f16 v74, v74, v61\n"
// fp16 transcendentals: plain (low word) and SDWA high word in place
#define EXH1 "v_exp_f16 v76, v76\n"
#define EXH2 EXH1 "v_log_f16 v77, v77\n"
#define EXH3 EXH2 "v_exp_f16 v78, v78\n"
#define EXS1 "v_exp_f16_sdwa v76, v76 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n"
#define EXS2 EXS1 "v_log_f16_sdwa v77, v77 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n"
#define EXS3 EXS2 "v_exp_f16_sdwa v78, v78 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n"
#define LH_LS "v_exp_f16 v76, v76\n" "v_exp_f16_sdwa v76, v76 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n"
// conversions
#define CVR1 "v_cvt_pkrtz_f16_f32 v79, v80, v81\n"
#define CVR2 CVR1 "v_cvt_pkrtz_f16_f32 v82, v83, v84\n"
#define CVN1 "v_cvt_pk_f16_f32 v79, v80, v81\n"
#define CVN2 CVN1 "v_cvt_pk_f16_f32 v82, v83, v84\n"
#define NONE ""

#define KSTEP(FILL, A0, N0, OFF)                                                          \
    "s_waitcnt lgkmcnt(0)\n"                                                               \
    "v_mfma_f32_32x32x16_f16 v[0:15], " A0 ", a[0:3], v[0:15]\n"                           \
    "ds_read_b128 " N0 ", %0 offset:" #OFF "\n" FILL

#define CLOB "a0","a1","a2","a3","v0","v1","v2","v3","v4","v5","v6","v7","v8","v9","v10","v11","v12","v13","v14","v15","v32","v33","v34","v35","v44","v45","v46","v47","v60","v61","v62","v63","v64","v65","v66","v67","v68","v69","v72","v73","v74","v75","v76","v77","v78","v79","v80","v81","v82","v83","v84"

#define KERNEL(NAME, FILL)                                                                                     \
    __global__ __launch_bounds__(256, 1) void NAME(unsigned long long* out, int iters) {                       \
        __shared__ __attribute__((aligned(16))) char lds[65536];                                               \
        const unsigned la = (threadIdx.x & 63) * 16;                                                           \
        asm volatile("s_waitcnt lgkmcnt(0)");                                                                  \
        unsigned long long t0 = __builtin_readcyclecounter();                                                  \
        for (int i = 0; i < iters; ++i)                                                                        \
            asm volatile(KSTEP(FILL, "v[32:35]", "v[44:47]", 0) KSTEP(FILL, "v[44:47]", "v[32:35]", 1024)      \
                         KSTEP(FILL, "v[32:35]", "v[44:47]", 2048) KSTEP(FILL, "v[44:47]", "v[32:35]", 3072)   \
                         ::"v"(la) : CLOB);                                                                    \
        asm volatile("s_nop 7\n s_nop 7");                                                                     \
        unsigned long long t1 = __builtin_readcyclecounter();                                                  \
        if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = t1 - t0;                                             \
        if (threadIdx.x == 12345) lds[threadIdx.x] = 1;                                                        \
    }

// the per-gap mixes of one tile's epilogue spread over 16 gaps: today 104 ops (32 transcendental) -> 6.5 per gap, ~2 of them
// transcendental; packed fp16 ~80 ops (32 transcendental) -> 5 per gap, 2 of them transcendental
KERNEL(k_none, NONE)
KERNEL(k_f1, FMA1) KERNEL(k_f2, FMA2) KERNEL(k_f3, FMA3) KERNEL(k_f4, FMA4) KERNEL(k_f5, FMA5)
KERNEL(k_e2, EXP2) KERNEL(k_e2f2, EXP2 FMA2) KERNEL(k_e2f3, EXP2 FMA3) KERNEL(k_e2f4, EXP2 FMA4) KERNEL(k_e2f5, EXP2 FMA5)
KERNEL(k_pm1, PKM1) KERNEL(k_pm2, PKM2) KERNEL(k_pm3, PKM3) KERNEL(k_pm4, PKM4)
KERNEL(k_pa1, PKA1) KERNEL(k_pa2, PKA2) KERNEL(k_pa3, PKA3)
KERNEL(k_pf1, PKF1) KERNEL(k_pf2, PKF2) KERNEL(k_pf3, PKF3) KERNEL(k_pf4, PKF4)
KERNEL(k_px1, PKX1) KERNEL(k_px2, PKX2) KERNEL(k_px3, PKX3)
KERNEL(k_eh1, EXH1) KERNEL(k_eh2, EXH2) KERNEL(k_eh3, EXH3)
KERNEL(k_es1, EXS1) KERNEL(k_es2, EXS2) KERNEL(k_es3, EXS3) KERNEL(k_lhls, LH_LS)
KERNEL(k_cr1, CVR1) KERNEL(k_cr2, CVR2) KERNEL(k_cn1, CVN1) KERNEL(k_cn2, CVN2)
KERNEL(k_eh2p2, EXH2 PKM1 PKA1) KERNEL(k_eh2p3, EXH2 PKM1 PKA1 PKX1) KERNEL(k_es2p3, EXS2 PKF1 PKA1 PKX1)
KERNEL(k_eh2p4, EXH2 PKM2 PKA1 PKX1)

int main() {
    unsigned long long* d;
    (void)hipMalloc(&d, 64);
    const int iters = 20000;
    struct { const char* name; void (*fn)(unsigned long long*, int); } ks[] = {
        {"no filler", k_none}, {"1 fma", k_f1}, {"2 fma", k_f2}, {"3 fma", k_f3}, {"4 fma", k_f4}, {"5 fma", k_f5},
        {"exp+log f32", k_e2}, {"exp+log f32 + 2 fma", k_e2f2}, {"exp+log f32 + 3 fma", k_e2f3}, {"exp+log f32 + 4 fma", k_e2f4},
        {"exp+log f32 + 5 fma", k_e2f5},
        {"1 pk_mul_f16", k_pm1}, {"2 pk_mul_f16", k_pm2}, {"3 pk_mul_f16", k_pm3}, {"4 pk_mul_f16", k_pm4},
        {"1 pk_add_f16", k_pa1}, {"2 pk_add_f16", k_pa2}, {"3 pk_add_f16", k_pa3},
        {"1 pk_fma_f16", k_pf1}, {"2 pk_fma_f16", k_pf2}, {"3 pk_fma_f16", k_pf3}, {"4 pk_fma_f16", k_pf4},
        {"1 pk_max_f16", k_px1}, {"2 pk_max_f16", k_px2}, {"3 pk_max_f16", k_px3},
        {"1 exp_f16", k_eh1}, {"exp+log f16", k_eh2}, {"exp+log+exp f16", k_eh3},
        {"1 exp_f16 sdwa hi", k_es1}, {"exp+log f16 sdwa hi", k_es2}, {"3 f16 sdwa hi", k_es3}, {"exp lo + exp sdwa hi", k_lhls},
        {"1 cvt_pkrtz", k_cr1}, {"2 cvt_pkrtz", k_cr2}, {"1 cvt_pk_f16_f32", k_cn1}, {"2 cvt_pk_f16_f32", k_cn2},
        {"exp+log f16 + pk_mul + pk_add", k_eh2p2}, {"exp+log f16 + mul, add, max pk", k_eh2p3},
        {"exp+log sdwa + fma, add, max pk", k_es2p3}, {"exp+log f16 + 4 pk", k_eh2p4}};
    for (auto& k : ks) {
        for (int rep = 0; rep < 2; ++rep) {
            hipLaunchKernelGGL(k.fn, dim3(256), dim3(256), 0, 0, d, iters);
            (void)hipDeviceSynchronize();
        }
        unsigned long long c = 0;
        (void)hipMemcpy(&c, d, 8, hipMemcpyDeviceToHost);
        printf("per MFMA gap: %-34s %.2f cycles per MFMA\n", k.name, (double)c / iters / 4);
    }
    return 0;
}
