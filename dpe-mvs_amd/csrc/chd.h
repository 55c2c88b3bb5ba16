// chd.h — DPE_CHD, the qualifier of the arithmetic the host shares with the kernels (fusion_world.h, cloud_dist.h
// and the headers built on them): host and device under hipcc, plain inline C++ under the host compiler.
#pragma once

#if defined(__HIPCC__)
#define DPE_CHD __host__ __device__ __forceinline__
#else
#define DPE_CHD inline
#endif
