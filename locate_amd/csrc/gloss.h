// The G-step's hinge arithmetic, shared by csrc/loss.hip (locate_g_loss) and csrc/topk.hip (locate_g_loss_topk, which with k = B has
// to return locate_g_loss's bits): the term of one logit and its gradient, each spelled ONCE here, as dloss.h does for the D-step.
//   g_error = mean( relu(1 - f_i) )        f = D(G(z));  float64 sum, rounded once to fp32
//   d g_error / d f_i = -(1 / n) where (1 - f_i) >= 0 (ATen's clamp backward mask: false for a NaN), else +0
#pragma once
#include "dloss.h"

__device__ __forceinline__ double g_hinge_term(float f) { return (double)hinge_clamp(1.0f - f); }

// whether the hinge passes a gradient at f
__device__ __forceinline__ bool g_hinge_passes(float f) { return (1.0f - f) >= 0.0f; }

// inv_n: 1.0f / (float)n, n the number of logits the mean runs over
__device__ __forceinline__ float g_hinge_grad(float f, float inv_n) { return g_hinge_passes(f) ? -inv_n : 0.0f; }

__device__ __forceinline__ float g_hinge_mean(double sum, int n) { return (float)(sum / n); }
