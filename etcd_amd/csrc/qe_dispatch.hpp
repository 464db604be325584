// qe_dispatch.hpp — declarations shared by the per-S instantiation objects
// (qe_inst.hip, qe_inst_prog.hip) and the C ABI (qe_api.hip).  Each
// dispatch_* is a function template over the slot count, defined in the .hip
// that holds its kernels and instantiated there for that object's QE_S;
// qe_api.hip picks the instantiation with with_slots (qe_launch.hpp).
#pragma once
#include "qe_kernels.hpp"
#include "qe_stream.hpp"
#include "qe_progress.hpp"
#include "qe_repl.hpp"

namespace qe {

int hip_status(hipError_t e);

// the Progress entry points that launch through dispatch_progress
enum class ProgressOp { Step, Send, CheckQuorum, ReadIndex, Propose, Heartbeat, SwitchConfig,
                        BecomeLeader };

template <int S>
int dispatch_cv(const CVArgs &a, int mode, bool vec, hipStream_t st);
template <int S>
int dispatch_repl(const RArgs &a, bool masked, bool joint, bool vec, hipStream_t st);
template <int S>
int dispatch_elec(const EArgs &a, hipStream_t st);
// acct: the instrumented variant with byte accounting (Step, Propose and
// SwitchConfig have one; measurement only)
template <int S>
int dispatch_progress(const PArgs &a, ProgressOp op, bool acct, bool masked, bool joint,
                      hipStream_t st);

}  // namespace qe
