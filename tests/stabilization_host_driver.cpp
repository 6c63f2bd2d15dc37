// Stand-alone driver of the host preparation of stabilize_frames (csrc/host/stabilization.hpp): the zoom mode by name, the order
// of the frames by time and the text of the plan file, with no device call.  tests/test_stabilization_restatement.py compiles it
// plain and with -fsanitize=address,undefined and compares what it prints with the Python twin.
//
//   stabilization_host_driver <zoom mode> <n> <t_1> .. <t_n> then per frame <name> <status> <w> <x> <y> <z> <required> <zoom> <clamped>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host/stabilization.hpp"

int main(int argc, char* argv[]) {
  namespace sth = OpenICC::stabilization;
  if (argc < 3) { std::fprintf(stderr, "usage: %s mode n times frames\n", argv[0]); return 2; }
  int mode = -1;
  if (sth::ZoomModeFromName(argv[1], &mode)) std::printf("mode %d\n", mode); else std::printf("mode refused\n");
  const int n = std::atoi(argv[2]);
  if (n < 0 || argc != 3 + n + 9 * n) { std::fprintf(stderr, "%d arguments for %d frames\n", argc, n); return 2; }
  std::vector<double> times;
  for (int k = 0; k < n; ++k) times.push_back(std::strtod(argv[3 + k], nullptr));
  std::printf("order");
  for (size_t i : sth::OrderByTime(times)) std::printf(" %zu", i);
  std::printf("\n");
  std::vector<std::string> names; std::vector<int32_t> status; std::vector<double> q, required, zoom; std::vector<uint8_t> clamped;
  for (int k = 0; k < n; ++k) {
    char** a = argv + 3 + n + 9 * k;
    names.push_back(a[0]); status.push_back(std::atoi(a[1]));
    for (int c = 0; c < 4; ++c) q.push_back(std::strtod(a[2 + c], nullptr));
    required.push_back(std::strtod(a[6], nullptr)); zoom.push_back(std::strtod(a[7], nullptr)); clamped.push_back(uint8_t(std::atoi(a[8])));
  }
  std::fputs(sth::PlanJson(names, status, q, required, zoom, clamped).c_str(), stdout);
  return 0;
}
