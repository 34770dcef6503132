// Host-side helpers shared by the one-shot device calls of libcaliscope_ba.so outside cba_lib.hip (cba_scale_errors, the cba_pose_*
// calls, cba_coverage_counts, cba_vertical_fit, cba_reprojection_filter, cba_reconstruct_trajectories): the error return, the device
// selection every call starts with, and the device buffers of one call.  Plain host C++ on six HIP calls, so that
// tests/native/device_call_check.cpp can run it against a stand-in for them.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/caliscope_ba.h"

namespace cba {
namespace {

int err(int code, const std::string& msg) { return cba_set_error(code, msg.c_str()); }  // returns `code`

// The device buffers of one call: freed on every path, typed, counted in elements, and sticky: after the first failure in(), make()
// and out() do nothing more (in / make return nullptr), so a call checks status() once before its first launch and once after its
// copy-backs.  A size is given as its factors (elements = their product), and elements * sizeof(T) is formed in bytes() alone.
struct Buffers {
  std::vector<void*> p;
  int rc = CBA_OK;
  std::string why;  // of the first failure

  Buffers() = default;
  Buffers(const Buffers&) = delete;
  Buffers& operator=(const Buffers&) = delete;
  ~Buffers() { for (void* b : p) (void)hipFree(b); }

  int status() const { return rc; }
  int result(const char* what) const { return rc ? err(rc, std::string(what) + ": " + why) : CBA_OK; }  // what the call returns
  void check(hipError_t e) {  // a launch or memset of the call: its failure is the call's, like a failed copy
    if (e != hipSuccess) set(CBA_ERR_HIP, hipGetErrorString(e));
  }

  // count elements, not uploaded; a zero count still gives a (8-byte) buffer: kernels are handed non-null pointers
  template <class T, class... N> T* make(N... count) { return (T*)alloc(bytes(sizeof(T), {(size_t)count...})); }
  // the same, with the elements of src uploaded (src == nullptr or a zero count: allocated only)
  template <class T, class... N> T* in(const T* src, N... count) {
    const size_t n = bytes(sizeof(T), {(size_t)count...});
    void* dst = alloc(n);
    if (dst && src && n && hipMemcpy(dst, src, n, hipMemcpyHostToDevice) != hipSuccess) return (T*)set(CBA_ERR_HIP, "device allocation / upload failed");
    return (T*)dst;
  }
  // count elements of dev back to host (host == nullptr or a zero count: nothing)
  template <class T, class... N> void out(T* host, const T* dev, N... count) {
    const size_t n = bytes(sizeof(T), {(size_t)count...});
    if (!rc && host && n) check(hipMemcpy(host, dev, n, hipMemcpyDeviceToHost));
  }

 private:
  void* set(int code, const char* msg) {
    if (!rc) { rc = code; why = msg; }
    return nullptr;
  }
  // elem * count[0] * count[1] * ..; 0, and CBA_ERR_UNSUPPORTED, when that does not fit size_t (a negative count arrives here as a huge one)
  size_t bytes(size_t elem, std::initializer_list<size_t> count) {
    size_t n = elem;
    for (size_t c : count)
      if (__builtin_mul_overflow(n, c, &n)) { set(CBA_ERR_UNSUPPORTED, "buffer size does not fit size_t"); return 0; }
    return n;
  }
  void* alloc(size_t n) {
    void* ptr = nullptr;
    if (rc) return nullptr;
    if (hipMalloc(&ptr, n > 8 ? n : 8) != hipSuccess) return set(CBA_ERR_HIP, "device allocation / upload failed");
    p.push_back(ptr);
    return ptr;
  }
};

int select_device(int32_t device, const char* what) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return err(CBA_ERR_NO_DEVICE, std::string(what) + ": no HIP device");
  if (device < 0 || device >= ndev) return err(CBA_ERR_INVALID, std::string(what) + ": device " + std::to_string(device) + " of " + std::to_string(ndev));
  if (hipSetDevice(device) != hipSuccess) return err(CBA_ERR_HIP, std::string(what) + ": hipSetDevice failed");
  return CBA_OK;
}

}  // namespace
}  // namespace cba
