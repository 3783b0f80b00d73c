// kernel_instances.h — which instantiations of the big kernel templates (kernels.h) live in which translation unit. api.hip only
// launches them: it sees `extern template` declarations (STHIP_DECLARE_KERNEL_INSTANCES) and the definitions are compiled, in
// parallel, in shade_*.hip and trace_kernels.hip (__graft_entry__.build_product): one hipcc process per file instead of four
// minutes of one. The lists themselves are in kernel_variants.h; api.hip launches through tables made from the same lists, so
// that an instantiation that is not listed cannot be launched (and so cannot be compiled into api.hip by accident).
#pragma once
#include "kernel_variants.h"
#include "kernels.h"

#define STHIP_SHADE_EXTERN(T, E, L, M, P, D) extern template __global__ void k_shade<T, E, L, M, P, D>(FrameParams, uint32_t);
#define STHIP_SHADE_DEFINE(T, E, L, M, P, D) template __global__ void k_shade<T, E, L, M, P, D>(FrameParams, uint32_t);
#define STHIP_TRACE_EXTERN(C, A, B, T, W) extern template __global__ void k_trace<C, A, B, T, W>(FrameParams, uint32_t, uint32_t);
#define STHIP_TRACE_DEFINE(C, A, B, T, W) template __global__ void k_trace<C, A, B, T, W>(FrameParams, uint32_t, uint32_t);
#define STHIP_LIGHT_EXTERN(T, E, M) extern template __global__ void k_shade_light<T, E, M>(FrameParams, uint32_t);
#define STHIP_LIGHT_DEFINE(T, E, M) template __global__ void k_shade_light<T, E, M>(FrameParams, uint32_t);

#define STHIP_DECLARE_KERNEL_INSTANCES \
  STHIP_SHADE_ALL(STHIP_SHADE_EXTERN) STHIP_TRACE_ALL(STHIP_TRACE_EXTERN) STHIP_SHADE_LIGHT(STHIP_LIGHT_EXTERN)
