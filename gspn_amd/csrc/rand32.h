// rand32.h -- gspn_roi_rand32 of include/gspn_hip.h on the device: the stateless counter-based generator shared by the ROI stage
// (roi.hip) and the instance resampling (sampling_segments.hip).
#pragma once

__device__ __forceinline__ unsigned long long roi_mix64(unsigned long long z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// the scene's stream: everything of gspn_roi_rand32 that does not depend on (a, b)
__device__ __forceinline__ unsigned long long roi_rand_scene(long long seed, int scene) {
    return roi_mix64((unsigned long long)seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(scene + 1));
}
__device__ __forceinline__ unsigned roi_rand32(unsigned long long scene_state, unsigned a, unsigned b) {
    return (unsigned)(roi_mix64(scene_state ^ (((unsigned long long)a << 32) | (unsigned long long)b)) >> 32);
}
