// masks.hip — the mask pre-pass of CEP_SESSION_MASK_PASS sessions.
//
// SURVEY Q9 (a strict, cardinality-ONE, fold-free pattern with distinct names emits a match at record j
// iff its key's k consecutive records j-k+1..j satisfy P1..Pk) does not depend on what the predicates
// read, as long as each is a pure function of the current record.  The stencil / chain kernels work on a
// per-record stage-mask byte; where the predicates do not lower to intervals of one column
// (compile.cpp analyse_stencil), this pass evaluates them per record through the shared bytecode
// machinery (interp.h) and writes the mask as an int32 column, which those kernels then read as their
// value column through the identity table (StencilProgram.lut[1 + m] = m).
//
// The built-in kernel here interprets; jit.cpp compiles the same body (masks_dev.h) per pattern.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "masks_dev.h"

namespace kcep {

__global__ __launch_bounds__(MK_THREADS) void masks_kernel(MaskArgs A) { masks_body(MaskInterpTab{A.P}, A); }

hipError_t masks_launch(const MaskArgs& A, hipStream_t st, hipFunction_t jf) {
  if (A.n <= 0) return hipSuccess;
  const int64_t groups = (A.n + 3) / 4;
  const unsigned blocks = unsigned(std::min<int64_t>((groups + MK_THREADS - 1) / MK_THREADS, MK_MAX_BLOCKS));
  if (jf) {
    MaskArgs a = A;
    void* args[] = {&a};
    return hipModuleLaunchKernel(jf, blocks, 1, 1, MK_THREADS, 1, 1, 0, st, args, nullptr);
  }
  hipLaunchKernelGGL(masks_kernel, dim3(blocks), dim3(MK_THREADS), 0, st, A);
  return hipGetLastError();
}

}  // namespace kcep
