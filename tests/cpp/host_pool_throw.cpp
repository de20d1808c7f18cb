// HostPool (manta_amd/csrc/host_pool.hpp): an exception thrown in a helper thread's share of a job reaches the caller, and the pool
// serves the next job.  Host only; built and run by tests/test_host_pool.py.
#include "host_pool.hpp"

#include <cstdio>
#include <numeric>
#include <stdexcept>
#include <string>

using namespace manta_host;

static int failures = 0;
static void expect(const bool ok, const char* what)
{
  if (!ok) {
    std::fprintf(stderr, "host_pool_throw: FAILED: %s\n", what);
    ++failures;
  }
}

/// the message of what hostParallel threw when `thrower` throws "part <t>" from its part(s); "" if nothing came out
static std::string thrownBy(const uint64_t n, const unsigned parts, const unsigned throwerMask)
{
  try {
    hostParallel(n, parts, [&](unsigned t, uint64_t, uint64_t) {
      if ((throwerMask >> t) & 1u) throw std::runtime_error("part " + std::to_string(t));
    });
  } catch (const std::runtime_error& e) {
    return e.what();
  }
  return "";
}

int main()
{
  setenv("MANTA_AMD_HOST_PARTS", "3", 1);
  const uint64_t n     = 1000;
  const unsigned parts = hostParts(n);
  expect(parts == 3, "MANTA_AMD_HOST_PARTS=3 gives three parts");

  expect(thrownBy(n, parts, 1u << 2) == "part 2", "a helper's exception arrives on the calling thread");

  std::vector<uint64_t> v(n);
  std::iota(v.begin(), v.end(), uint64_t(1));
  uint64_t sum[3] = {0, 0, 0};
  hostParallel(n, parts, [&](unsigned t, uint64_t a, uint64_t z) { sum[t] = std::accumulate(v.begin() + a, v.begin() + z, uint64_t(0)); });
  expect(sum[0] && sum[1] && sum[2], "every part ran");
  expect(sum[0] + sum[1] + sum[2] == n * (n + 1) / 2, "the job after a failed one sums the whole range");

  expect(thrownBy(n, parts, 1u << 0) == "part 0", "the caller's own part throws");
  expect(thrownBy(n, parts, (1u << 0) | (1u << 1)) == "part 0", "the caller's own exception wins over a helper's");
  expect(thrownBy(n, parts, 0) == "", "nothing is left over for the next job");

  if (!failures) std::printf("host_pool_throw ok\n");
  return failures ? 1 : 0;
}
