// Error type and per-thread last-error message of the C-ABI (include/kgs.h: every entry point
// returns a KGS_E_* code, kgs_last_error() the message of the calling thread's last failure).
// Host-only; shared by the prover (prover.cpp and the other C-ABI units) and the host-only units (ptau_io.cpp, verifier.cpp).
#pragma once
#include <stdexcept>
#include <string>

namespace kgs {

struct KgsError : std::runtime_error {
  int code;
  KgsError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// the calling thread's last-error slot (defined in ptau_io.cpp)
std::string& kgs_errbuf();

inline int kgs_fail(const KgsError& e) {
  kgs_errbuf() = e.what();
  return e.code;
}

}  // namespace kgs

// The error boundary of a C-ABI entry point whose failures are the device's (KGS_E_HIP for anything that
// is not a KgsError): `API_BEGIN body API_END` returns KGS_OK unless the body returns or throws. The codes
// come from include/kgs.h at the place of use.
#define API_BEGIN try {
#define API_END                     \
  }                                 \
  catch (const KgsError& e) {       \
    return kgs_fail(e);             \
  }                                 \
  catch (const std::exception& e) { \
    kgs_errbuf() = e.what();        \
    return KGS_E_HIP;               \
  }                                 \
  return KGS_OK;
