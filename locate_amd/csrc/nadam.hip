// Fused multi-tensor Nadam step (reference libs/nadam.py:31-89; hyper-parameters libs/config.py:70-73).
// The reference loops over ~100 parameter tensors in Python with ~10 ATen calls each; here one tiny
// "schedule" kernel advances every tensor's (step, m_schedule) state ON DEVICE (so the whole optimizer step
// can live inside a captured hipGraph) and one streaming kernel updates all tensors.
//
// Per tensor (state is per tensor because tensors whose gradient is None are skipped, nadam.py:44-45):
//   t <- t + 1
//   mc_t   = b1 (1 - 0.5 * 0.96^(t sd)),  mc_t1 = b1 (1 - 0.5 * 0.96^((t+1) sd))
//   ms_new = m_schedule * mc_t,  ms_next = ms_new * mc_t1,  m_schedule <- ms_new
//   g <- g + weight_decay p   (nadam.py:65-66; 0 in the reference's training loop)
//   m <- b1 m + (1-b1) g ;  v <- b2 v + (1-b2) g^2 ;  denom = sqrt(v / (1 - b2^t)) + eps
//   p <- p - lr (1-mc_t)/(1-ms_new) * g / denom ;  p <- p - lr mc_t1/(1-ms_next) * m / denom
// The bodies are nadam_step.h's, shared with the guarded step (guard.hip): every rounding of an element's update is spelled out there.
#include "nadam_step.h"

__global__ void __launch_bounds__(64) nadam_schedule_kernel(const NadamTensor* __restrict__ tensors, NadamCoef* __restrict__ coef,
                                                            int n_tensors, double lr, double b1, double b2, double sd) {
    nadam_schedule(tensors, coef, n_tensors, lr, b1, b2, sd, true);
}

__global__ void __launch_bounds__(256) nadam_update_kernel(const NadamTensor* __restrict__ tensors,
                                                           const NadamCoef* __restrict__ coef,
                                                           const int2* __restrict__ chunks, float b1, float b2, float eps, float wd) {
    nadam_update<false>(tensors, coef, chunks, b1, b2, eps, wd, 0, 1.0f);
}

LOCATE_API size_t locate_nadam_tensor_record_bytes(void) { return sizeof(NadamTensor); }
LOCATE_API int locate_nadam_chunk_elems(void) { return MT_CHUNK; }

// tensors: DEVICE array of n_tensors records {p, g, m, v, sched, n, absmax (nullable)}; coef: DEVICE scratch of n_tensors * 16 bytes;
// chunks: DEVICE array of n_chunks (tensor index, chunk index) int pairs covering every tensor in
// locate_nadam_chunk_elems() pieces.
LOCATE_API int locate_nadam_step(const void* tensors, void* coef, const void* chunks, int n_tensors, int n_chunks, double lr,
                                 double beta1, double beta2, double eps, double schedule_decay, double weight_decay, void* stream) {
    LOCATE_REQUIRE(tensors && coef && chunks && n_tensors > 0 && n_chunks > 0, "locate_nadam_step: bad arguments");
    hipStream_t st = as_stream(stream);
    nadam_schedule_kernel<<<(n_tensors + 63) / 64, 64, 0, st>>>(static_cast<const NadamTensor*>(tensors),
                                                               static_cast<NadamCoef*>(coef), n_tensors, lr, beta1, beta2,
                                                               schedule_decay);
    LOCATE_LAUNCH_CHECK("locate_nadam_step(schedule)");
    nadam_update_kernel<<<n_chunks, 256, 0, st>>>(static_cast<const NadamTensor*>(tensors), static_cast<const NadamCoef*>(coef),
                                                  static_cast<const int2*>(chunks), (float)beta1, (float)beta2, (float)eps,
                                                  (float)weight_decay);
    LOCATE_LAUNCH_CHECK("locate_nadam_step(update)");
    return LOCATE_OK;
}
