// fa2_regfile.h -- the C++ side of the register file that the generated main-loop bodies (*.inc) own.
//
// A kernel with a generated body is compiled with amdgpu_num_vgpr(n): hipcc allocates v0..v(n-1); every VGPR above and the
// whole accumulator file are named literally by the bodies.  The statements here are how compiler code seeds, reads and
// rescales those registers around the bodies -- each instruction pattern exists once; a call site names the shape of its
// kernel's register file and the clobber class of the statement.
//
// Shape:  RF512  one wave per SIMD: 256 VGPRs + 256 AGPRs          RF128  two waves per SIMD: 128 + 128
//
// Clobber class -- PART OF A STATEMENT'S BEHAVIOUR: a wider or narrower list moves hipcc's code around the statement, and in
// kernels that leave hipcc 32 - 64 registers that decides between fitting and spilling.  Do not change a site's class without
// comparing the assembly (tools/asm_identity.py).
//   CL_TOP    the file's top VGPR.  Never allocated by hipcc, so the clobber costs nothing; naming it is what makes the kernel
//             descriptor cover the whole file (the register count is taken from the highest register mentioned).
//   CL_ACC    the accumulator list alone: keeps hipcc out of the AGPRs (no operand parked there, no copy through them) across
//             the statement.  Every statement that writes an accumulator has at least this.  The backward kernels use it
//             bare: with the top VGPR added, hipcc sees a register dependence between an accumulator write and the
//             CL_TOP statement behind it and pads them with an s_nop.
//   CL_FILE   both: the whole body-owned file (the fp8 forward's seeding statements).
//   CL_ORDER  + "memory", vcc, scc, m0 and the bodies' scratch SGPRs, i.e. the bodies' own list: orders the statement against
//             the bodies like one of them (the bf16 forward, whose seeding statements sit between bodies on the restart path).
// Reads (vget, aread) clobber nothing.
#pragma once
#include "fa2_common.h"

namespace fa2 {

#define FA2_ACC_LO \
    "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", \
    "a16", "a17", "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", \
    "a32", "a33", "a34", "a35", "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", \
    "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", \
    "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73", "a74", "a75", "a76", "a77", "a78", "a79", \
    "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", "a91", "a92", "a93", "a94", "a95", \
    "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106", "a107", "a108", "a109", "a110", "a111", \
    "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124", "a125", "a126", "a127"
#define FA2_ACC_HI \
    "a128", "a129", "a130", "a131", "a132", "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140", "a141", "a142", "a143", \
    "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156", "a157", "a158", "a159", \
    "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175", \
    "a176", "a177", "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191", \
    "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207", \
    "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222", "a223", \
    "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237", "a238", "a239", \
    "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252", "a253", "a254", "a255"
#define FA2_ACC512 FA2_ACC_LO, FA2_ACC_HI
#define FA2_ACC128 FA2_ACC_LO
#define FA2_RF512 "v255", FA2_ACC512
#define FA2_RF128 "v127", FA2_ACC128
#define FA2_RF_MISC "memory", "vcc", "scc", "s10", "s11", "s12", "m0"

enum { RF512 = 512, RF128 = 128 };
enum { CL_TOP, CL_ACC, CL_FILE, CL_ORDER };

// One asm statement, compiled with the clobber list of (shape, class).  Operand lists contain commas: write them with FA2_COMMA.
#define FA2_RF_ASM(RF, CL, TEXT, OUTS, INS)                                                                     \
    do {                                                                                                         \
        static_assert(((RF) == RF512 || (RF) == RF128) && (CL) >= CL_TOP && (CL) <= CL_ORDER, "register-file shape and clobber class"); \
        if constexpr ((RF) == RF512 && (CL) == CL_TOP) asm volatile(TEXT : OUTS : INS : "v255");                      \
        else if constexpr ((RF) == RF512 && (CL) == CL_ACC) asm volatile(TEXT : OUTS : INS : FA2_ACC512);             \
        else if constexpr ((RF) == RF512 && (CL) == CL_FILE) asm volatile(TEXT : OUTS : INS : FA2_RF512);             \
        else if constexpr ((RF) == RF512) asm volatile(TEXT : OUTS : INS : FA2_RF_MISC, FA2_RF512);                 \
        else if constexpr ((CL) == CL_TOP) asm volatile(TEXT : OUTS : INS : "v127");                                \
        else if constexpr ((CL) == CL_ACC) asm volatile(TEXT : OUTS : INS : FA2_ACC128);                              \
        else if constexpr ((CL) == CL_FILE) asm volatile(TEXT : OUTS : INS : FA2_RF128);                            \
        else asm volatile(TEXT : OUTS : INS : FA2_RF_MISC, FA2_RF128);                                            \
    } while (0)
#define FA2_COMMA ,

// ---- literal VGPR v[R]: set (any 32-bit value) and get
template <int RF, int CL, int R, typename T>
__device__ __forceinline__ void vset(T x)
{
    static_assert(sizeof(T) == 4, "one register");
    FA2_RF_ASM(RF, CL, "v_mov_b32 v%c1, %0", , "v"(x) FA2_COMMA "i"(R));
}
template <int R>
__device__ __forceinline__ float vget()
{
    float x;
    asm volatile("v_mov_b32 %0, v%c1" : "=v"(x) : "i"(R));
    return x;
}

// ---- literal AGPR a[R].  The asm is opaque to hipcc's hazard recogniser: any non-MFMA access to a register an MFMA may
// still be writing must be preceded by mfma_acc_settle().
__device__ __forceinline__ void mfma_acc_settle()
{
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
}
template <int RF, int CL, int R, typename T>
__device__ __forceinline__ void awrite(T x)
{
    static_assert(sizeof(T) == 4, "one register");
    FA2_RF_ASM(RF, CL, "v_accvgpr_write_b32 a[%c1], %0", , "v"(x) FA2_COMMA "i"(R));
}
template <int R>
__device__ __forceinline__ float aread()
{
    float x;
    asm volatile("v_accvgpr_read_b32 %0, a[%c1]" : "=v"(x) : "i"(R));
    return x;
}
// Parks a bf16x8 fragment (an MFMA operand that never changes during the kernel) in a[LO : LO+3].
template <int RF, int CL, int LO>
__device__ __forceinline__ void awrite_frag(bf16x8 f)
{
    const u32x4 w = __builtin_bit_cast(u32x4, f);
    FA2_RF_ASM(RF, CL, "v_accvgpr_write_b32 a[%c4], %0\n\tv_accvgpr_write_b32 a[%c5], %1\n\t"
                       "v_accvgpr_write_b32 a[%c6], %2\n\tv_accvgpr_write_b32 a[%c7], %3", ,
               "v"(w[0]) FA2_COMMA "v"(w[1]) FA2_COMMA "v"(w[2]) FA2_COMMA "v"(w[3]) FA2_COMMA "i"(LO) FA2_COMMA "i"(LO + 1)
                   FA2_COMMA "i"(LO + 2) FA2_COMMA "i"(LO + 3));
}
// a[R : R+3] *= alpha (per lane)
template <int RF, int CL, int R>
__device__ __forceinline__ void ascale4(float alpha)
{
    float t0, t1, t2, t3;
    FA2_RF_ASM(RF, CL, "v_accvgpr_read_b32 %0, a[%c5]\n\tv_accvgpr_read_b32 %1, a[%c6]\n\t"
                       "v_accvgpr_read_b32 %2, a[%c7]\n\tv_accvgpr_read_b32 %3, a[%c8]\n\t"
                       "v_mul_f32 %0, %0, %4\n\tv_mul_f32 %1, %1, %4\n\tv_mul_f32 %2, %2, %4\n\tv_mul_f32 %3, %3, %4\n\t"
                       "v_accvgpr_write_b32 a[%c5], %0\n\tv_accvgpr_write_b32 a[%c6], %1\n\t"
                       "v_accvgpr_write_b32 a[%c7], %2\n\tv_accvgpr_write_b32 a[%c8], %3",
               "=&v"(t0) FA2_COMMA "=&v"(t1) FA2_COMMA "=&v"(t2) FA2_COMMA "=&v"(t3),
               "v"(alpha) FA2_COMMA "i"(R) FA2_COMMA "i"(R + 1) FA2_COMMA "i"(R + 2) FA2_COMMA "i"(R + 3));
}
// a[R : R+15] = 0: one MFMA on a zero fragment instead of 16 accumulator writes.  (hipcc does not know the statement is an
// MFMA: the wait states between its write of z and the read are the s_nop.)
template <int RF, int CL, int R>
__device__ __forceinline__ void azero16(u32x4 z)
{
    FA2_RF_ASM(RF, CL, "s_nop 1\n\tv_mfma_f32_32x32x16_bf16 a[%c1:%c2], %0, %0, 0", , "v"(z) FA2_COMMA "i"(R) FA2_COMMA "i"(R + 15));
}

}  // namespace fa2
