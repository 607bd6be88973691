// Loss glue of the training step (reference main.py:149-156,164-169, libs/utils.py:133-134,
// libs/grad_penalty.py:1-2): scalars from [B] vectors, one small block.  Values AND the gradients with
// respect to the discriminator outputs come out of the same launch, so the step driver can start the
// backward passes directly from them.
//   D-step:  d_error = mean( relu(1 - t_i) + relu(1 + f_i) )        t = D(real), f = D(G(z).detach())
//            penalty = gamma * (mean t - mean a)^2                   a = D(augmented real)   (not a gradient penalty)
//   G-step:  g_error = mean( relu(1 - f_i) )
// clamp(min=0) passes the gradient where its argument is >= 0 (ATen clamp backward mask).
#include "dloss.h"
#include "gloss.h"

// the arithmetic lives in dloss.h, which csrc/lecam.hip shares, and in gloss.h, which csrc/topk.hip shares
__global__ void __launch_bounds__(256) d_loss_kernel(const float* __restrict__ t, const float* __restrict__ f,
                                                     const float* __restrict__ a, int B, float gamma, float* __restrict__ losses,
                                                     float* __restrict__ gt, float* __restrict__ gf, float* __restrict__ ga) {
    __shared__ double scratch[16];
    d_loss_plain(t, f, a, B, gamma, losses, gt, gf, ga, scratch);
}

__global__ void __launch_bounds__(256) g_loss_kernel(const float* __restrict__ f, int B, float* __restrict__ loss,
                                                     float* __restrict__ gf) {
    __shared__ double scratch[16];
    double hs = 0.0;
    const float invB = 1.0f / (float)B;
    for (int i = threadIdx.x; i < B; i += blockDim.x) {
        hs += g_hinge_term(f[i]);
        gf[i] = g_hinge_grad(f[i], invB);
    }
    hs = block_sum<double>(hs, scratch);
    if (threadIdx.x == 0) loss[0] = g_hinge_mean(hs, B);
}

// losses: 3 floats {d_error, penalty, d_error + penalty};  g_*: [B] gradients of the total w.r.t. each D output
LOCATE_API int locate_d_loss(const float* d_true, const float* d_fake, const float* d_aug, int B, float gamma, float* losses,
                             float* g_true, float* g_fake, float* g_aug, void* stream) {
    LOCATE_REQUIRE(B > 0 && d_true && d_fake && d_aug && losses && g_true && g_fake && g_aug, "locate_d_loss: bad arguments");
    d_loss_kernel<<<1, 256, 0, as_stream(stream)>>>(d_true, d_fake, d_aug, B, gamma, losses, g_true, g_fake, g_aug);
    LOCATE_LAUNCH_CHECK("locate_d_loss");
    return LOCATE_OK;
}

LOCATE_API int locate_g_loss(const float* d_fake, int B, float* loss, float* g_fake, void* stream) {
    LOCATE_REQUIRE(B > 0 && d_fake && loss && g_fake, "locate_g_loss: bad arguments");
    g_loss_kernel<<<1, 256, 0, as_stream(stream)>>>(d_fake, B, loss, g_fake);
    LOCATE_LAUNCH_CHECK("locate_g_loss");
    return LOCATE_OK;
}
