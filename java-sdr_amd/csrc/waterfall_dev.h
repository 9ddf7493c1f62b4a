// waterfall_dev.h -- waterfall.paintLine / getMax (waterfall.java:87-109) on the device, stated once: k_waterfall
// (formats.hip) pools a PSD row read from memory, k_fft_pix (fft_psd.hip) the row its own last pass left in LDS.
#pragma once
#include "common.h"

namespace jsdr {

// Java (int) of a float: truncate toward zero, saturate, NaN -> 0
__device__ __forceinline__ int java_f2i(float v)
{
    if (v != v) return 0;
    if (v >= 2147483648.0f) return 2147483647;
    if (v <= -2147483648.0f) return (-2147483647 - 1);
    return (int)v;
}

// waterfall.java:89: float step = (float)n / width
__device__ __forceinline__ float wf_step(int n, int width) { return (float)n / (float)width; }

// waterfall.java:102-109 getMax over bins [o, o + l) of a row read through at(i): '>' never replaces with or by a NaN,
// and l <= 0 takes bin o alone
template <class AT>
__device__ __forceinline__ float wf_getmax(AT at, int o, int l)
{
    float r = at(o);
    for (int i = o + 1; i < o + l; i++) {
        const float v = at(i);
        if (v > r) r = v;
    }
    return r;
}

// the peak colour 0xRRGGBB, taken apart once per kernel
struct WfColour {
    int r, g, b;
};
__device__ __forceinline__ WfColour wf_colour(unsigned peak_rgb)
{
    return WfColour{(int)((peak_rgb >> 16) & 0xff), (int)((peak_rgb >> 8) & 0xff), (int)(peak_rgb & 0xff)};
}

// waterfall.java:91-99: 255 - (int)(m * -2.55f), clamped to 0..255, scaled into the peak colour with /256, alpha 0xff
__device__ __forceinline__ unsigned wf_pixel(float m, const WfColour &c)
{
    int f = 255 - java_f2i(m * -2.55f);
    f = f < 0 ? 0 : f;
    f = f > 255 ? 255 : f;
    const unsigned cr = (unsigned)(c.r * f / 256), cg = (unsigned)(c.g * f / 256), cb = (unsigned)(c.b * f / 256);
    return 0xff000000u | (cr << 16) | (cg << 8) | cb;
}

}  // namespace jsdr
