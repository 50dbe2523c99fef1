// Context and profiler (see runtime.hpp).
#include "runtime.hpp"

namespace lbf {

Ctx::~Ctx() {
  comm.reset();
  if (own_stream && stream) (void)hipStreamDestroy(stream);
}

Profiler::~Profiler() {
  for (auto e : pool) (void)hipEventDestroy(e);
}

size_t Profiler::mark(hipStream_t s) {
  if (used == pool.size()) {
    hipEvent_t e;
    LBF_HIP(hipEventCreateWithFlags(&e, hipEventDefault | event_release_flags()));
    pool.push_back(e);
  }
  LBF_HIP(hipEventRecord(pool[used], s));
  return used++;
}

void Profiler::add(const Rec &r, float t) {
  if (size_t(r.id) >= ms.size()) {
    ms.resize(r.id + 1, 0.0);
    cnt.resize(r.id + 1, 0);
    work.resize(r.id + 1, 0.0);
  }
  ms[r.id] += t;
  cnt[r.id] += 1;
  work[r.id] += r.work;
}

void Profiler::resolve() {
  if (recs.empty()) return;
  LBF_HIP(hipEventSynchronize(pool[used - 1]));
  for (auto &r : recs) {
    float t = 0.f;
    LBF_HIP(hipEventElapsedTime(&t, pool[r.a], pool[r.b]));
    add(r, t);
  }
  recs.clear();
  used = 0;
}

void Profiler::merge_into(Profiler &dst) {
  resolve();
  if (dst.ms.size() < ms.size()) {
    dst.ms.resize(ms.size(), 0.0);
    dst.cnt.resize(ms.size(), 0);
    dst.work.resize(ms.size(), 0.0);
  }
  for (size_t i = 0; i < ms.size(); ++i) {
    dst.ms[i] += ms[i];
    dst.cnt[i] += cnt[i];
    dst.work[i] += work[i];
  }
  ms.assign(ms.size(), 0.0);
  cnt.assign(cnt.size(), 0);
  work.assign(work.size(), 0.0);
}

void Ctx::set_device() const { LBF_HIP(hipSetDevice(device)); }

void Ctx::allreduce(float *buf, size_t count) {
  if (!dp()) return;
  comm->allreduce(buf, count, stream);
}

} // namespace lbf
