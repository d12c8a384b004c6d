// float_keys.h -- floats as integers that order like them, so that a minimum or a maximum of floats can land with an integer atomicMin /
// atomicMax: nearest.hip (the bounds of a scene) and components.hip (the box of a mask row).
#pragma once

// floats to integers that order like them (-0 below +0, which is harmless here); the reset values decode to NaN
__device__ __forceinline__ int np_key(float x) { const int v = __float_as_int(x); return v >= 0 ? v : v ^ 0x7FFFFFFF; }
__device__ __forceinline__ float np_unkey(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7FFFFFFF); }
