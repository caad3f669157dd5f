// The structs behind the C ABI's opaque handles (include/april_api.h, include/aprilx_engine.h), stated once for april_api.cc and every
// *_api.cc: each of those files is a translation unit of its own (the scheduler harness builds only some of them), all of them see
// the same definitions.
#pragma once
#include <memory>
#include <vector>
#include "../../include/april_api.h"
#include "../../include/aprilx_engine.h"
#include "bias.h"
#include "lm.h"
#include "session.h"

struct AprilASRModel_i { aprilx::Model m; };
struct AprilASRSession_i { aprilx::Session s; };
struct AprilxBias_i { std::shared_ptr<const aprilx::BiasSet> set; };
struct AprilxLm_i { std::shared_ptr<const aprilx::LmSet> lm; };
struct AprilxGreedy_i {
    aprilx::Greedy g; AprilRecognitionResultHandler handler; void *ud; std::vector<aprilx::Event> ev;
    void flush_events() { aprilx::deliver_events(ev, aprilx::Handlers{handler, ud}); }
};
