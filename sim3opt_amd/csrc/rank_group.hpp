// rank_group.hpp -- the ranks one process drives (sim3opt_set_devices with n > 1).
//
// The caller stays single-threaded: the handle owns n rank contexts, each an Engine, a Comm of the in-process
// transport (comm_local.hip) and a persistent worker thread bound to the rank's device (HIP's current device is per
// thread).  A public call posts ONE command to all workers and returns when every rank has finished it.  A rank whose
// command fails aborts the group's barrier before it returns, so that its peers leave their collectives with
// SIM3OPT_ERR_COMM instead of waiting for it; the group is finished then (broken()), and only its destruction is left.
#pragma once

#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "comm.hpp"
#include "engine.hpp"

namespace sim3opt {

struct RankCtx {
  int32_t rank = 0, device = 0;
  Engine* engine = nullptr;
  Comm comm;        // handed to the engine at initialize, taken back before a re-initialisation
  bool connected = false;  // peer access enabled (once)
  std::string err;  // of the last command
  int rc = 0;
  std::vector<sim3opt_iter_stats> stats;
  std::vector<sim3opt_tr_stats> tr_stats;
};

class RankGroup {
 public:
  RankGroup(int32_t n, const int32_t* devices, double timeout_s);
  ~RankGroup();  // releases the engines under their own devices, then joins the workers
  RankGroup(const RankGroup&) = delete;
  RankGroup& operator=(const RankGroup&) = delete;

  int32_t size() const { return (int32_t)ctx_.size(); }
  RankCtx& ctx(int32_t r) { return ctx_[r]; }
  const RankCtx& ctx(int32_t r) const { return ctx_[r]; }
  bool broken() const { return local_.barrier.aborted(); }

  // f(ctx) on every rank's worker (on rank 0's only with all == false).  A negative value is a failure.  Returns the
  // value of the lowest failing rank and its message in `err`, else rank 0's.
  int run(const std::function<int(RankCtx&)>& f, std::string& err, bool all = true);

 private:
  void worker(int32_t r);

  LocalGroup local_;
  std::vector<RankCtx> ctx_;
  std::vector<std::thread> threads_;
  std::mutex mu_;
  std::condition_variable cv_work_, cv_done_;
  const std::function<int(RankCtx&)>* job_ = nullptr;
  bool job_all_ = true;
  uint64_t posted_ = 0;  // commands so far
  int32_t pending_ = 0;  // workers that have not finished the current one
  bool stop_ = false;
};

}  // namespace sim3opt
