// The host copy engine of the host-buffer boundary (host_copy.cpp): copies between pageable caller
// buffers and pinned staging, split over a pool of host threads. No HIP here: the caller enqueues every
// DMA, so the unit runs without a device (tests/native/host_copy_check.cpp, under sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <functional>
#include <vector>

namespace kgsi {

struct CopyJob {
  uint8_t* dst;
  const uint8_t* src;
  size_t len;
};
void par_copy(const std::vector<CopyJob>& jobs);
// one vector into pinned staging; ready(offset, len) on the calling thread per `dma`-byte span, in
// order, once that span is copied
void stream_copy(uint8_t* dst, const uint8_t* src, size_t len, size_t dma, const std::function<void(size_t, size_t)>& ready);

// A kgs_prove call in progress in the process, for as long as the object lives: a copy made while more
// than one is alive uses non-temporal stores (host_copy.cpp copy_nt_now).
struct ProofInProgress {
  ProofInProgress();
  ~ProofInProgress();
};

}  // namespace kgsi
