// Internal interface between wgrad.hip (the router and the C-ABI entry points) and the kernel families it routes to.
#pragma once
#include "common.hpp"
#include "../../include/abcnet_hip.h"

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

__device__ inline bf16x8 tr_read8(const char* base0, const char* base1) {
    bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)base0);
    bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)base1);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// heads' 1x1 weight gradient (wgrad_heads.hip)
int abc_wgrad_head_ok(const abc_wgrad_desc* d);
int abc_wgrad_head_launch(const abc_wgrad_desc* d, abc_stream_t stream);

// weight gradient against a one-channel operand (wgrad_c1.hip)
int abc_wgrad_c1_ok(const abc_wgrad_desc* d);
int abc_wgrad_c1_launch(const abc_wgrad_desc* d, abc_stream_t stream);
