// rtrec_amd/csrc/factor_als.hip.h -- what rtrec_factor_gram / rtrec_factor_gram_wide (factor_gram.hip), rtrec_factor_als_solve
// (factor_als.hip) and rtrec_factor_als_cg (factor_als_cg.hip) share: the dim limits, the chunk of the Gram contract, the tile
// classes and the accumulator's element map.
#pragma once
#include "common.hip.h"
#include "../../include/rtrec_amd_ext.h"

namespace rtrec {

typedef float als_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kAlsMaxDim = 64;            // dim limit of both calls: one 32 x 32 tile up to 32, the three lower tiles up to 64
constexpr int kAlsWideMaxDim = 256;       // dim limit of rtrec_factor_gram_wide and rtrec_factor_als_cg: what the factor scorer serves
constexpr int kAlsGramChunk = 1024;      // rows of V per partial Gram: a CONTRACT constant (include/rtrec_amd_ext.h)
constexpr int kAlsGroup = 8;              // k-steps whose operand loads are issued together, ahead of their chain

// row of a 32 x 32 tile that accumulator register g of this lane holds (the column is lane & 31)
__device__ __forceinline__ int als_acc_row(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

}  // namespace rtrec
