// What the two meter kernels share (metrics.hip: the training flavour of train.py:145-215; eval_tables.hip: the inference
// flavour of test_accuracy.py:188-269): the 24 distinct sums behind the 17 meters, their (numerator, denominator) slots and
// the small device helpers both per-pixel passes use.
//   slots 0-4 / 5-9  atom / bond centres: peak & target, peak & dil3(target), peaks, target & dil3(peak), targets
//   10-15            atom types / charges / hs: matched mass, mass
//   16-18            bond types: matched mass, mass; rho: sum |rho| error * mass
//   19-23            omega: target & temp, temp, target & circ3(temp), targets, circ3(target) & temp
#pragma once
#include <hip/hip_runtime.h>

constexpr int ABC_METER_NSUM = 24;
constexpr int ABC_METER_COUNT = 17;

// meter -> (numerator slot, denominator slot); order = METER_NAMES of oracle/metrics_oracle.py
__device__ inline int abc_meter_num_slot(int meter) {
    const int ni[ABC_METER_COUNT] = {0, 1, 0, 3, 10, 12, 14, 5, 6, 5, 8, 16, 18, 19, 21, 19, 23};
    return ni[meter];
}
__device__ inline int abc_meter_den_slot(int meter) {
    const int di[ABC_METER_COUNT] = {2, 2, 4, 4, 11, 13, 15, 7, 7, 9, 9, 17, 17, 20, 22, 22, 20};
    return di[meter];
}

__device__ inline double abc_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ inline unsigned long long abc_circ3(unsigned long long m) {  // 60-bit circular dilation by one bin either way
    const unsigned long long M60 = (1ull << 60) - 1;
    return (m | ((m << 1) & M60) | (m >> 59) | (m >> 1) | ((m & 1ull) << 59)) & M60;
}
