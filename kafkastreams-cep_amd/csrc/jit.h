// jit.h — per-pattern kernels (jit.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>

#include "kcep_internal.h"

namespace kcep {

// One pattern's specialised kernels, loaded from a code object hiprtc built.
// Shared by every session of the same program text (process-wide cache).
struct JitModule {
  hipModule_t mod = nullptr;
  hipFunction_t runs_sim = nullptr;     // runs_dev.h runs_sim_body<JitTab>
  hipFunction_t runs_write = nullptr;   // runs_dev.h runs_write_body<JitTab>
  hipFunction_t nfa = nullptr;          // nfa_dev.h nfa_kernel_body (general path)
  hipFunction_t nfa_wave = nullptr;     // nfa_wave.h nfa_wave_body, one key per wave (general path)
  hipFunction_t nfa_order = nullptr;    // nfa_dev.h nfa_order_bits_body, the wave kernel's schedule estimate
  hipFunction_t masks = nullptr;        // masks_dev.h masks_body<MaskJitTab>, the mask pre-pass
  hipFunction_t follow_bits = nullptr;  // follow_bits_dev.h follow_eval_bits_body<MaskJitTab>, the follow path's evaluated form
  ~JitModule();
};

// The HIP source of the pattern's runs kernels: the DevProgram as a constexpr
// table plus every predicate / fold as straight-line code (empty + why if some
// bytecode cannot be translated).
std::string jit_source_runs(const Program& P, std::string& why);

// Compile (or fetch from the cache) and load the runs kernels; nullptr + why on failure.
std::shared_ptr<const JitModule> jit_runs(const Program& P, std::string& why);

// Generate and compile only (no device needed): false + why if either fails.
bool jit_check_runs(const Program& P, std::string& why);

// the same for the general NFA path's kernel (nfa_dev.h)
std::string jit_source_general(const Program& P, std::string& why, bool phases = false, bool stop = false);
// phases: the profiling build (KCEP_PHASES clocks, CEP_SESSION_PROFILE sessions); stop: the kernels'
// CEP_BATCH_STOP_AT_ERROR build, a module of its own that only flagged batches compile and launch
std::shared_ptr<const JitModule> jit_general(const Program& P, std::string& why, bool phases = false, bool stop = false);
bool jit_check_general(const Program& P, std::string& why);

// the same for the mask pre-pass of a mask-pass eligible pattern (masks_dev.h); follow: of a pattern in the
// follow path's evaluated form (Program::follow_mask_prog), which KCEP_FOLLOW_MASK_SPLIT=1 sessions run
std::string jit_source_masks(const Program& P, std::string& why, bool follow = false);
std::shared_ptr<const JitModule> jit_masks(const Program& P, std::string& why, bool follow = false);
bool jit_check_masks(const Program& P, std::string& why);

// the same for the streaming kernel of the follow path's evaluated form (follow_bits_dev.h)
// (many: of Program::follow_many_prog, a CEP_SESSION_FOLLOW_MANY session's)
std::string jit_source_follow_bits(const Program& P, std::string& why, bool many = false);
std::shared_ptr<const JitModule> jit_follow_bits(const Program& P, std::string& why, bool many = false);
bool jit_check_follow_bits(const Program& P, std::string& why);

}  // namespace kcep
