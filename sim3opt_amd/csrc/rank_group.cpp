// rank_group.cpp -- worker threads of the ranks one process drives (see rank_group.hpp).
#include "rank_group.hpp"

#include <hip/hip_runtime.h>

namespace sim3opt {

RankGroup::RankGroup(int32_t n, const int32_t* devices, double timeout_s) : ctx_((size_t)n) {
  local_.world = n;
  local_.timeout_s = timeout_s > 0.0 ? timeout_s : 120.0;
  local_.barrier.reset_parties(n);
  for (int32_t r = 0; r < n; ++r) {
    ctx_[r].rank = r;
    ctx_[r].device = devices[r];
    local_.ranks[r].device = devices[r];
    comm_init_local(ctx_[r].comm, &local_, r);
  }
  threads_.reserve((size_t)n);
  for (int32_t r = 0; r < n; ++r) threads_.emplace_back(&RankGroup::worker, this, r);
}

RankGroup::~RankGroup() {
  std::string ignored;
  // a rank that failed may have left launches behind that store into a peer's mailbox: everything is quiet before
  // any mailbox goes
  if (broken()) run([](RankCtx&) { (void)hipDeviceSynchronize(); return 0; }, ignored);
  run([](RankCtx& c) {
    if (c.engine) engine_destroy(c.engine);  // (gives the engine's communicator and its mailboxes back)
    c.engine = nullptr;
    c.comm.release();
    return 0;
  }, ignored);
  {
    std::lock_guard<std::mutex> lk(mu_);
    stop_ = true;
  }
  cv_work_.notify_all();
  for (std::thread& t : threads_) t.join();
}

int RankGroup::run(const std::function<int(RankCtx&)>& f, std::string& err, bool all) {
  {
    std::unique_lock<std::mutex> lk(mu_);
    job_ = &f;
    job_all_ = all;
    pending_ = size();
    ++posted_;
    cv_work_.notify_all();
    cv_done_.wait(lk, [&] { return pending_ == 0; });
    job_ = nullptr;
  }
  for (const RankCtx& c : ctx_)
    if (c.rc < 0) {
      err = c.err;
      return c.rc;
    }
  if (!ctx_[0].err.empty()) err = ctx_[0].err;
  return ctx_[0].rc;
}

void RankGroup::worker(int32_t r) {
  RankCtx& c = ctx_[r];
  (void)hipSetDevice(c.device);  // (a bad ordinal was refused by sim3opt_set_devices; the engine checks again)
  uint64_t seen = 0;
  for (;;) {
    const std::function<int(RankCtx&)>* job = nullptr;
    bool mine = true, all = true;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_work_.wait(lk, [&] { return stop_ || posted_ != seen; });
      if (posted_ == seen) return;  // (stop, and nothing left to do)
      seen = posted_;
      job = job_;
      all = job_all_;
      mine = all || r == 0;
    }
    c.err.clear();
    c.rc = 0;
    if (mine) {
      try {
        c.rc = (*job)(c);
      } catch (...) {  // (std::bad_alloc ...: nothing leaves the thread)
        c.rc = SIM3OPT_ERR_ARG;
        c.err = "rank " + std::to_string(r) + ": out of host memory or internal error";
      }
      // the peers may be inside a collective this rank will never join
      if (c.rc < 0 && all) local_.barrier.abort();
    }
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (--pending_ == 0) cv_done_.notify_all();
    }
  }
}

}  // namespace sim3opt
