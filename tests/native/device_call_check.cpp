// caliscope_amd/csrc/device_call.h against the stand-in HIP of tests/native/fake_hip: the buffers of a one-shot device call under a
// failure injected at every allocation and every copy, their success path, and select_device.  A program of its own (built with
// -fsanitize=address,undefined by tests/test_device_call.py): prints what failed and exits 1, or exits 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "device_call.h"

static int g_code = 0;
static std::string g_message;
extern "C" int cba_set_error(int32_t code, const char* message) {
  g_code = code;
  g_message = message ? message : "";
  return code;
}

static int g_failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("%s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, g_case); \
      ++g_failures;                                                      \
    }                                                                    \
  } while (0)
static char g_case[64] = "";

static void reset_fake() { fake_hip() = FakeHip(); }

// A call's worth of buffers: five allocations, two uploads, then three copy-backs (and one into a null host pointer).  Unlike an
// entry point it does not return at the first failure: every later request must turn into nothing by itself.
constexpr int N_ALLOC = 5, N_UPLOAD = 2, N_COPY = 5;
constexpr double SENTINEL = -777.0;
struct Host {
  double a[5] = {1.5, -2.5, 3.25, 4.0, 1e300};
  int64_t b[6] = {0, 1, -2, 3, INT64_MAX, INT64_MIN};
  double a_back[5];
  int64_t b_back[6];
  int32_t n_back[7];
  const void* dev[N_ALLOC];
  Host() {
    for (double& v : a_back) v = SENTINEL;
    for (int64_t& v : b_back) v = (int64_t)SENTINEL;
    for (int32_t& v : n_back) v = (int32_t)SENTINEL;
  }
};
static int sequence(Host& h) {
  cba::Buffers buf;
  double* da = buf.in(h.a, 5);
  int64_t* db = buf.in(h.b, 3, 2);
  double* dwork = buf.make<double>(4);
  int32_t* dzero = buf.make<int32_t>(0);
  int32_t* dn = buf.in((const int32_t*)nullptr, 7);  // no source: allocated only
  const void* dev[N_ALLOC] = {da, db, dwork, dzero, dn};
  std::memcpy(h.dev, dev, sizeof dev);
  if (!buf.status())
    for (int i = 0; i < 7; ++i) dn[i] = 100 + i;  // (the kernel)
  buf.out(h.a_back, da, 5);
  buf.out(h.b_back, db, 3, 2);
  buf.out((double*)nullptr, dwork, 4);  // nobody asked for it
  buf.out(h.n_back, dn, 7);
  return buf.result("seq");
}

static bool untouched(const Host& h, bool a, bool b, bool n) {
  bool ok = true;
  if (a) for (double v : h.a_back) ok = ok && v == SENTINEL;
  if (b) for (int64_t v : h.b_back) ok = ok && v == (int64_t)SENTINEL;
  if (n) for (int32_t v : h.n_back) ok = ok && v == (int32_t)SENTINEL;
  return ok;
}

static void check_injected_failures() {
  for (int k = 1; k <= N_ALLOC; ++k) {
    std::snprintf(g_case, sizeof g_case, "allocation %d fails", k);
    reset_fake();
    fake_hip().fail_malloc = k;
    Host h;
    g_code = 0;
    const int rc = sequence(h);
    const FakeHip& f = fake_hip();
    CHECK(rc == CBA_ERR_HIP && g_code == CBA_ERR_HIP);
    CHECK(g_message == "seq: device allocation / upload failed");
    CHECK(f.mallocs == k);                              // nothing after the failure reached the allocator
    CHECK(f.copies == (k - 1 < N_UPLOAD ? k - 1 : N_UPLOAD));  // .. or the copy: only the uploads before it
    CHECK(untouched(h, true, true, true));
    for (int i = 0; i < N_ALLOC; ++i) CHECK((h.dev[i] != nullptr) == (i < k - 1));
    CHECK(f.frees == k - 1 && f.bad_frees == 0 && f.live.empty());  // every block before k freed exactly once
  }
  for (int k = 1; k <= N_COPY; ++k) {
    std::snprintf(g_case, sizeof g_case, "copy %d fails", k);
    reset_fake();
    fake_hip().fail_copy = k;
    Host h;
    g_code = 0;
    const int rc = sequence(h);
    const FakeHip& f = fake_hip();
    CHECK(rc == CBA_ERR_HIP && g_code == CBA_ERR_HIP);
    CHECK(g_message.rfind("seq: ", 0) == 0);
    CHECK(f.copies == k);
    const int allocated = k <= N_UPLOAD ? k : N_ALLOC;  // a failed upload leaves its own block allocated, and is the last request served
    CHECK(f.mallocs == allocated);
    for (int i = 0; i < N_ALLOC; ++i) CHECK((h.dev[i] != nullptr) == (i < (k <= N_UPLOAD ? k - 1 : N_ALLOC)));
    CHECK(untouched(h, k <= 3, k <= 4, true));
    if (k > 3) CHECK(std::memcmp(h.a_back, h.a, sizeof h.a) == 0);
    if (k > 4) CHECK(std::memcmp(h.b_back, h.b, sizeof h.b) == 0);
    CHECK(f.frees == allocated && f.bad_frees == 0 && f.live.empty());
  }
}

static void check_success_path() {
  std::snprintf(g_case, sizeof g_case, "success");
  reset_fake();
  {
    Host h;
    g_code = 12345;
    CHECK(sequence(h) == CBA_OK && g_code == 12345);  // no error was set
    const FakeHip& f = fake_hip();
    CHECK(f.mallocs == N_ALLOC && f.copies == N_COPY);  // the copy-back into a null host pointer never reached the stand-in
    CHECK(std::memcmp(h.a_back, h.a, sizeof h.a) == 0 && std::memcmp(h.b_back, h.b, sizeof h.b) == 0);
    for (int i = 0; i < 7; ++i) CHECK(h.n_back[i] == 100 + i);
    for (int i = 0; i < N_ALLOC; ++i) CHECK(h.dev[i] != nullptr);  // the zero-size request included
    CHECK(f.frees == N_ALLOC && f.bad_frees == 0 && f.live.empty());
  }
  std::snprintf(g_case, sizeof g_case, "zero count");
  reset_fake();
  {
    cba::Buffers buf;
    const double one = 1.0;
    double host = SENTINEL;
    double* d0 = buf.in(&one, 0);
    CHECK(d0 != nullptr && fake_hip().last_malloc_bytes == 8 && fake_hip().copies == 0);
    double* d1 = buf.make<double>(3, 0);
    CHECK(d1 != nullptr && d1 != d0 && fake_hip().last_malloc_bytes == 8);
    buf.out(&host, d0, 0);
    CHECK(host == SENTINEL && fake_hip().copies == 0 && buf.status() == CBA_OK);
  }
  CHECK(fake_hip().frees == 2 && fake_hip().live.empty());
  std::snprintf(g_case, sizeof g_case, "overflow");
  const size_t top = std::numeric_limits<size_t>::max();
  const struct { size_t n0, n1; } big[] = {{top / 4, 1}, {top, 1}, {(size_t)1 << 40, (size_t)1 << 40}, {(size_t)-5, 3}};
  for (const auto& c : big) {
    reset_fake();
    {
      cba::Buffers buf;
      double* keep = buf.make<double>(2);
      CHECK(keep != nullptr && fake_hip().mallocs == 1);
      CHECK(buf.make<double>(c.n0, c.n1) == nullptr);
      CHECK(buf.status() == CBA_ERR_UNSUPPORTED && fake_hip().mallocs == 1);  // refused before the allocator
      CHECK(buf.make<double>(2) == nullptr && fake_hip().mallocs == 1);       // and sticky
      g_code = 0;
      CHECK(buf.result("big") == CBA_ERR_UNSUPPORTED && g_code == CBA_ERR_UNSUPPORTED && g_message.rfind("big: ", 0) == 0);
    }
    CHECK(fake_hip().frees == 1 && fake_hip().bad_frees == 0 && fake_hip().live.empty());
  }
  std::snprintf(g_case, sizeof g_case, "check");
  reset_fake();
  {
    cba::Buffers buf;
    double host = SENTINEL;
    double* d = buf.make<double>(1);
    buf.check(hipSuccess);
    CHECK(buf.status() == CBA_OK);
    buf.check(hipErrorInvalidValue);  // a failed launch: the copy-backs after it do nothing
    buf.check(hipErrorOutOfMemory);   // (the first failure stays)
    buf.out(&host, d, 1);
    CHECK(buf.status() == CBA_ERR_HIP && host == SENTINEL && fake_hip().copies == 0);
    CHECK(buf.result("launch") == CBA_ERR_HIP && g_message == "launch: invalid argument");
  }
}

static void check_select_device() {
  std::snprintf(g_case, sizeof g_case, "select_device");
  reset_fake();
  fake_hip().device_count = 0;
  CHECK(cba::select_device(0, "caller_a") == CBA_ERR_NO_DEVICE && g_code == CBA_ERR_NO_DEVICE && g_message.rfind("caller_a: ", 0) == 0);
  reset_fake();
  fake_hip().count_fails = true;
  CHECK(cba::select_device(0, "caller_a") == CBA_ERR_NO_DEVICE && g_message.rfind("caller_a: ", 0) == 0);
  reset_fake();
  fake_hip().device_count = 2;
  CHECK(cba::select_device(2, "caller_b") == CBA_ERR_INVALID && g_code == CBA_ERR_INVALID && g_message == "caller_b: device 2 of 2");
  CHECK(cba::select_device(-1, "caller_b") == CBA_ERR_INVALID && g_message.rfind("caller_b: ", 0) == 0);
  CHECK(fake_hip().selected == -1);
  g_code = 12345;
  CHECK(cba::select_device(1, "caller_c") == CBA_OK && g_code == 12345 && fake_hip().selected == 1);
  fake_hip().select_fails = true;
  CHECK(cba::select_device(0, "caller_d") == CBA_ERR_HIP && g_message.rfind("caller_d: ", 0) == 0);
}

int main() {
  check_injected_failures();
  check_success_path();
  check_select_device();
  if (g_failures) std::printf("%d checks failed\n", g_failures);
  else std::printf("device_call.h: all checks passed\n");
  return g_failures ? 1 : 0;
}
