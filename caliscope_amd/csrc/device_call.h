// Host-side helpers shared by the one-shot device calls of libcaliscope_ba.so (pose_lib.hip, scale_lib.hip): the error return, the
// device buffers of one call, and the device selection every call starts with.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/caliscope_ba.h"

namespace cba {
namespace {

int err(int code, const std::string& msg) { return cba_set_error(code, msg.c_str()); }  // returns `code`

// device buffers of one call, freed on every path
struct Buffers {
  std::vector<void*> p;
  ~Buffers() { for (void* b : p) (void)hipFree(b); }
  int up(const void* src, size_t bytes, void** dst) {
    void* ptr = nullptr;
    if (hipMalloc(&ptr, std::max<size_t>(bytes, 8)) != hipSuccess) return CBA_ERR_HIP;
    p.push_back(ptr);
    if (src && bytes && hipMemcpy(ptr, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return CBA_ERR_HIP;
    *dst = ptr;
    return CBA_OK;
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
