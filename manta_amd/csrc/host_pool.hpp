// Host loops over a whole batch (validation scan of the offset arrays, compaction of the results) split over a few threads.  Standard
// library and getpid() only: tests/cpp/host_pool_throw.cpp compiles this header alone.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>
#include <unistd.h>
#include <vector>

namespace manta_host {

static const unsigned kHostPartsMax = 8;
inline unsigned hostParts(const uint64_t n)
{
  static const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  if (const char* forced = std::getenv("MANTA_AMD_HOST_PARTS"))  // tests: take the multi-range paths on small batches too
    return unsigned(std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(n, kHostPartsMax), uint64_t(std::max(1, std::atoi(forced))))));
  if (n < 4096) return 1;
  return std::min(n < 262144 ? 4u : kHostPartsMax, hw);  // (eight for the passes over every read of a large batch)
}
/// seven helper threads per process, parked on a condition variable between jobs (starting std::threads per call costs more
/// than the loops they would share on a 256-core host)
class HostPool {
 public:
  static HostPool& get()
  {
    static HostPool pool;
    return pool;
  }
  /// fn(part, begin, end) for `parts` (<= kHostPartsMax) contiguous ranges of [0, n); part 0 runs on the caller's thread.  One job at a
  /// time: concurrent callers (workers of a batch call) queue up behind runMu.  An exception of fn leaves through here once every part
  /// has finished: the caller's own if part 0 threw, else the first a helper caught.
  template <typename F>
  void run(const uint64_t n, const unsigned parts, F fn)
  {
    auto begin = [&](unsigned t) { return n * t / parts; };
    if (parts <= 1 || getpid() != owner) {  // (a fork()ed child has no helper threads: it runs the loop itself)
      fn(0u, uint64_t(0), n);
      return;
    }
    std::lock_guard<std::mutex> only(runMu);
    std::function<void(unsigned)> job = [&](unsigned t) { fn(t, begin(t), begin(t + 1)); };
    {
      std::lock_guard<std::mutex> g(mu);
      current = &job;
      wanted  = parts - 1;
      pending = parts - 1;
      ++generation;
    }
    cv.notify_all();
    std::exception_ptr thrown;  // (fn may throw on the caller's part: the helpers still hold a pointer to `job`, so they are waited for first)
    try {
      fn(0u, begin(0), begin(1));
    } catch (...) {
      thrown = std::current_exception();
    }
    {
      std::unique_lock<std::mutex> g(mu);
      done.wait(g, [&] { return pending == 0; });
      current = nullptr;
      if (!thrown) thrown = failure;
      failure = nullptr;
    }
    if (thrown) std::rethrow_exception(thrown);
  }

 private:
  HostPool() : owner(getpid())
  {
    for (unsigned i = 0; i + 1 < kHostPartsMax; ++i) threads.emplace_back([this, i] { loop(i + 1); });
  }
  ~HostPool()
  {
    if (getpid() != owner) {  // fork()ed child: the threads do not exist here
      for (std::thread& t : threads) t.detach();
      return;
    }
    {
      std::lock_guard<std::mutex> g(mu);
      stop = true;
    }
    cv.notify_all();
    for (std::thread& t : threads) t.join();
  }
  void loop(const unsigned id)
  {
    uint64_t seen = 0;
    while (true) {
      std::function<void(unsigned)>* job = nullptr;
      {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return stop || generation != seen; });
        if (stop) return;
        seen = generation;
        if (id <= wanted) job = current;
      }
      if (job) {
        std::exception_ptr thrown;
        try {
          (*job)(id);
        } catch (...) {
          thrown = std::current_exception();
        }
        std::lock_guard<std::mutex> g(mu);
        if (thrown && !failure) failure = thrown;
        if (--pending == 0) done.notify_one();
      }
    }
  }
  const pid_t                    owner;
  std::mutex                     mu, runMu;
  std::condition_variable        cv, done;
  std::vector<std::thread>       threads;
  std::function<void(unsigned)>* current = nullptr;
  unsigned                       wanted = 0, pending = 0;
  uint64_t                       generation = 0;
  std::exception_ptr             failure;  // the first exception a helper caught in the current job
  bool                           stop = false;
};
template <typename F>
void hostParallel(const uint64_t n, const unsigned parts, F fn)
{
  HostPool::get().run(n, parts, fn);
}

}  // namespace manta_host
