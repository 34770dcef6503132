// A stand-in for the six HIP calls of caliscope_amd/csrc/device_call.h on host memory, for tests/native/device_call_check.cpp: put
// this directory first on the include path and `#include <hip/hip_runtime.h>` finds it.  Every call is counted, the k-th allocation
// or the k-th copy can be made to fail, and every block is tracked from hipMalloc to hipFree.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <map>

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2, hipErrorNoDevice = 100, hipErrorInvalidDevice = 101 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };

struct FakeHip {
  int mallocs = 0, copies = 0, frees = 0;          // calls that reached the stand-in
  int fail_malloc = 0, fail_copy = 0;              // the k-th such call fails (1-based; 0: none)
  int bad_frees = 0;                               // hipFree of a pointer that is not a live block (a second free included)
  std::map<void*, size_t> live;                    // blocks allocated and not yet freed, with the size asked for
  size_t last_malloc_bytes = 0;
  int device_count = 1, selected = -1;
  bool count_fails = false, select_fails = false;
};
inline FakeHip& fake_hip() {
  static FakeHip state;
  return state;
}

inline hipError_t hipMalloc(void** ptr, size_t bytes) {
  FakeHip& f = fake_hip();
  f.last_malloc_bytes = bytes;
  if (++f.mallocs == f.fail_malloc) return hipErrorOutOfMemory;
  *ptr = std::malloc(bytes);  // exactly the size asked for: the sanitizer sees a copy that runs past it
  f.live[*ptr] = bytes;
  return hipSuccess;
}
template <class T> hipError_t hipMalloc(T** ptr, size_t bytes) { return hipMalloc((void**)ptr, bytes); }

inline hipError_t hipFree(void* ptr) {
  FakeHip& f = fake_hip();
  ++f.frees;
  if (!f.live.erase(ptr)) { ++f.bad_frees; return hipErrorInvalidValue; }
  std::free(ptr);
  return hipSuccess;
}

inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  FakeHip& f = fake_hip();
  if (++f.copies == f.fail_copy) return hipErrorInvalidValue;
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}

inline hipError_t hipGetDeviceCount(int* n) {
  if (fake_hip().count_fails) return hipErrorNoDevice;
  *n = fake_hip().device_count;
  return hipSuccess;
}
inline hipError_t hipSetDevice(int device) {
  if (fake_hip().select_fails) return hipErrorInvalidDevice;
  fake_hip().selected = device;
  return hipSuccess;
}
inline const char* hipGetErrorString(hipError_t e) {
  switch (e) {
    case hipSuccess: return "no error";
    case hipErrorInvalidValue: return "invalid argument";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorNoDevice: return "no ROCm-capable device is detected";
    default: return "invalid device ordinal";
  }
}
