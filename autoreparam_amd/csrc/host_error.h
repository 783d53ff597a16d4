// What every translation unit needs on the host: error reporting (arp_last_error) and the gate of the experiment and test
// switches.  The diagnostics and probe.hip include this alone; the sampler's plumbing is host_common.h, which includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>

namespace arp {

void set_error(const std::string& msg);

#define ARP_HIP_OK(expr)                                                          \
  do {                                                                            \
    hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess) {                                                       \
      ::arp::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));        \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

// The one gate of the library's experiment and test switches: the value of the environment variable `name`, honoured under
// ARP_DEBUG=1 only and announced on stderr -- a stray variable must not change which kernel a production run takes, and says
// that it was ignored.  nullptr: unset, empty or ignored.  `note` ends the announcement; `said` (a switch that is asked for
// on every call but announces itself once per process) holds whether it has.
inline const char* debug_switch(const char* name, const char* note = "", bool* said = nullptr) {
  const char* e = getenv(name);
  if (!e || !e[0]) return nullptr;
  const char* d = getenv("ARP_DEBUG");
  if (!(d && d[0] == '1' && d[1] == 0)) {
    fprintf(stderr, "libautoreparam_hip: %s=%s IGNORED (experiment switch; set ARP_DEBUG=1 to enable it)\n", name, e);
    return nullptr;
  }
  if (!(said && *said)) fprintf(stderr, "libautoreparam_hip: DEBUG SWITCH %s=%s is in effect%s\n", name, e, note);
  if (said) *said = true;
  return e;
}
// integer experiment switch
inline bool debug_int(const char* name, int* out) {
  const char* e = debug_switch(name);
  if (e) *out = atoi(e);
  return e != nullptr;
}

}  // namespace arp
