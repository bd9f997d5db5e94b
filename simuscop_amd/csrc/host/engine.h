// host/engine.h -- the engine context as simuReads, seqToProfile and truthEval hold it.
#pragma once
#include <string>

#include "../../../include/simuscop_amd.h"
#include "common.h"

namespace simu {

struct Engine {  // RAII around sg_ctx (sg_destroy ends a training or evaluation session first), turns status codes into simu::Error
  sg_ctx* ctx = nullptr;
  ~Engine() { if (ctx) sg_destroy(ctx); }
  void check(int rc, const char* what) const {
    if (rc != SG_OK) throw Error(std::string("GPU engine error in ") + what + ": " + sg_last_error(ctx));
  }
};

}  // namespace simu
