// rank_barrier.hpp -- the host barrier of the ranks one process drives (rank_group.hpp, Comm::kind == 3).
//
// A generation-counting barrier on std::mutex / std::condition_variable with two ways out besides "everybody
// arrived": abort() releases every waiter, now and from then on, and a waiter that has waited longer than its
// timeout aborts the barrier itself.  Either way nobody hangs on a rank that failed or never arrives.  An
// aborted barrier stays aborted: the group it belongs to is finished.  No HIP in here (tests/cxx/rank_barrier_driver.cpp
// runs it under ThreadSanitizer).
#pragma once

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>

namespace sim3opt {

class RankBarrier {
 public:
  enum Result { PASSED = 0, ABORTED = 1, TIMED_OUT = 2 };

  explicit RankBarrier(int parties = 1) : parties_(parties) {}
  RankBarrier(const RankBarrier&) = delete;
  RankBarrier& operator=(const RankBarrier&) = delete;

  void reset_parties(int parties) {  // (before any thread waits)
    std::lock_guard<std::mutex> lk(mu_);
    parties_ = parties;
  }

  // PASSED: all parties arrived (what each of them wrote before its wait is visible to all after it).
  // ABORTED: somebody called abort(), or another waiter timed out.  TIMED_OUT: this caller waited longer than
  // timeout_s; it has aborted the barrier for the others.
  Result wait(double timeout_s) {
    std::unique_lock<std::mutex> lk(mu_);
    if (aborted_) return ABORTED;
    const unsigned long long gen = generation_;
    if (++arrived_ == parties_) {
      arrived_ = 0;
      ++generation_;
      cv_.notify_all();
      return PASSED;
    }
    // The limit is kept on the steady clock; the waits themselves are short system-clock slices, because that form
    // of the timed wait is pthread_cond_timedwait, which ThreadSanitizer follows (the steady-clock form is not
    // intercepted by every libtsan, which then loses track of the mutex).  A clock jump costs one slice at most.
    using steady = std::chrono::steady_clock;
    const steady::time_point deadline =
        steady::now() + std::chrono::duration_cast<steady::duration>(std::chrono::duration<double>(timeout_s));
    while (generation_ == gen && !aborted_) {
      const steady::duration left = deadline - steady::now();
      if (left <= steady::duration::zero()) {
        aborted_ = true;
        cv_.notify_all();
        return TIMED_OUT;
      }
      const auto slice = std::min<steady::duration>(left, std::chrono::milliseconds(100));
      cv_.wait_until(lk, std::chrono::system_clock::now() + slice);
    }
    // (a generation that completed counts even when an abort followed it before this thread woke up)
    return generation_ != gen ? PASSED : ABORTED;
  }

  void abort() {
    std::lock_guard<std::mutex> lk(mu_);
    aborted_ = true;
    cv_.notify_all();
  }

  bool aborted() const {
    std::lock_guard<std::mutex> lk(mu_);
    return aborted_;
  }

 private:
  mutable std::mutex mu_;
  std::condition_variable cv_;
  int parties_;
  int arrived_ = 0;
  unsigned long long generation_ = 0;
  bool aborted_ = false;
};

// what a rank reports when wait() did not pass, `seq` being the collective's sequence number on that rank
inline std::string rank_barrier_message(RankBarrier::Result how, int rank, double timeout_s, unsigned long long seq) {
  if (how == RankBarrier::TIMED_OUT)
    return "rank " + std::to_string(rank) + " waited longer than " + std::to_string(timeout_s) +
           " s for its peers in collective " + std::to_string(seq) + " (the group is finished)";
  return "rank " + std::to_string(rank) + ": collective " + std::to_string(seq) +
         " abandoned, another rank failed or timed out (the group is finished)";
}

}  // namespace sim3opt
