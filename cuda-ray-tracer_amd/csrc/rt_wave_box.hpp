// rt_wave_box.hpp -- the FP32 bounding box of up to 64 points held one per lane, rounded outwards, wave-uniform.
// Used by both schedules of rt_wavefront.hip (a block's hits; a chunk's hits) and, alone, by rt_debug_wave_box (rt_wave_box.hip).
// The box only feeds conservative culling: what matters is that it contains every used point and that it is the same box everywhere.
#ifndef RT_WAVE_BOX_HPP
#define RT_WAVE_BOX_HPP

#include <hip/hip_runtime.h>

// RT_WAVE_BOX_LIBRARY_ROUNDING=1 takes the device library's __double2float_rd / __double2float_ru (about 17 instructions each: convert,
// integer ulp step, compares, selects) instead of the rounding-mode conversions below; the values are the same (tests/test_wave_box_gpu.py).
#ifndef RT_WAVE_BOX_LIBRARY_ROUNDING
#define RT_WAVE_BOX_LIBRARY_ROUNDING 0
#endif

// lo[a] = min, hi[a] = max over the lanes with `use` of coordinate a rounded to FP32 towards -inf / +inf (the largest float <= v, the
// smallest float >= v); (+inf, -inf) when no lane is used.  Every lane of the wave must be active; the results are wave-uniform (scalar
// registers).
//   * Rounding: v_cvt_f32_f64 under the MODE register's rounding fields -- bits 1:0 round FP32 results, bits 3:2 FP64 / FP16 ones (0 nearest
//     even, 1 towards +inf, 2 towards -inf).  Both fields are set, so it does not matter which of them the hardware consults for a
//     conversion between the two widths; the denormal bits (7:4) are not touched.  A kernel starts with both fields 0 and nothing in this
//     project leaves them otherwise, so 0 is what is restored.  Everything is ONE asm statement: no other floating-point instruction can be
//     scheduled between the s_setreg instructions.
//   * Lanes without `use` carry +inf / -inf, selected (v_cndmask on the ballot of `use`), not branched: all six chains run in every lane.
//   * One network: per DPP step six independent v_min_f32 / v_max_f32 with the DPP modifier on the instruction itself and dst = src
//     (lanes without a valid source, and rows the row_mask leaves out, keep their own value).  Steps: the quad's other lanes, the row's
//     other quads (row_ror:4, row_ror:8: every lane has its row of 16), row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3;
//     lane 63 then holds the wave's value.  36 instructions.  Written through the compiler's DPP builtin, each step came out as v_mov_b32 +
//     s_nop + v_mov_b32_dpp + a canonicalising v_max_f32 + the v_min / v_max, five instructions, and the six reductions ran one behind
//     the other, each behind a branch of its own.
//   * min / max are exact, the inputs are conversion results (never signalling NaNs), and the kernels run with the IEEE mode bit set: a
//     quiet NaN operand gives the other operand, so the result is fminf / fmaxf over the lanes -- a NaN coordinate drops out of the box
//     as before (every culling comparison against that lane is made per lane, where NaN compares false and the sphere stays).
//   * Hazards (inline assembly gets no automatic nops).  Two s_setreg of one register need two wait states between them: three
//     conversions stand between the first and the second, the whole network behind the third.  A DPP instruction may read a VGPR two
//     wait states after a VALU instruction wrote it at the earliest, and five wait states after a VALU instruction wrote EXEC: between
//     two steps of a chain, and between a chain's select and its first step, stand the five other chains; in front of the first step
//     stand the fifteen instructions of the rounding and seeding part.  So the statement holds no s_nop.  (With the library's roundings there is
//     no such prefix, and one s_nop 4 in front of the first step covers both hazards.)
__device__ __forceinline__ void wave_box_f32(bool use, double x, double y, double z, float lo[3], float hi[3])
{
    const float inf = __builtin_inff();
    float a0, a1, a2, b0, b1, b2;
#define RT_BOX_STEP(CTRL)                    \
    "v_min_f32_dpp %0, %0, %0 " CTRL "\n\t" \
    "v_min_f32_dpp %1, %1, %1 " CTRL "\n\t" \
    "v_min_f32_dpp %2, %2, %2 " CTRL "\n\t" \
    "v_max_f32_dpp %3, %3, %3 " CTRL "\n\t" \
    "v_max_f32_dpp %4, %4, %4 " CTRL "\n\t" \
    "v_max_f32_dpp %5, %5, %5 " CTRL "\n\t"
#define RT_BOX_NETWORK                                             \
    RT_BOX_STEP("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf") \
    RT_BOX_STEP("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf") \
    RT_BOX_STEP("row_ror:4 row_mask:0xf bank_mask:0xf")           \
    RT_BOX_STEP("row_ror:8 row_mask:0xf bank_mask:0xf")           \
    RT_BOX_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf")        \
    RT_BOX_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")
#if RT_WAVE_BOX_LIBRARY_ROUNDING
    a0 = use ? __double2float_rd(x) : inf; a1 = use ? __double2float_rd(y) : inf; a2 = use ? __double2float_rd(z) : inf;
    b0 = use ? __double2float_ru(x) : -inf; b1 = use ? __double2float_ru(y) : -inf; b2 = use ? __double2float_ru(z) : -inf;
    asm volatile("s_nop 4\n\t" RT_BOX_NETWORK : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(b0), "+v"(b1), "+v"(b2));
#else
    const unsigned long long used = __ballot(use);
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 4), 0xa\n\t"
                 "v_cvt_f32_f64 %0, %6\n\t"
                 "v_cvt_f32_f64 %1, %7\n\t"
                 "v_cvt_f32_f64 %2, %8\n\t"
                 "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 4), 0x5\n\t"
                 "v_cvt_f32_f64 %3, %6\n\t"
                 "v_cvt_f32_f64 %4, %7\n\t"
                 "v_cvt_f32_f64 %5, %8\n\t"
                 "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 4), 0x0\n\t"
                 "v_cndmask_b32_e64 %0, %9, %0, %10\n\t"
                 "v_cndmask_b32_e64 %1, %9, %1, %10\n\t"
                 "v_cndmask_b32_e64 %2, %9, %2, %10\n\t"
                 "v_cndmask_b32_e64 %3, -%9, %3, %10\n\t"
                 "v_cndmask_b32_e64 %4, -%9, %4, %10\n\t"
                 "v_cndmask_b32_e64 %5, -%9, %5, %10\n\t"
                 RT_BOX_NETWORK
                 : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(b0), "=&v"(b1), "=&v"(b2)
                 : "v"(x), "v"(y), "v"(z), "v"(inf), "s"(used));
#endif
#undef RT_BOX_NETWORK
#undef RT_BOX_STEP
    // read-out through the builtin: the compiler sees these v_readlane_b32 and keeps their own hazards
    lo[0] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a0), 63));
    lo[1] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a1), 63));
    lo[2] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a2), 63));
    hi[0] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b0), 63));
    hi[1] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b1), 63));
    hi[2] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b2), 63));
}

#endif
