// gg_host.h - host-only pieces every translation unit with entry points shares: the device-switch guard and the compute
// unit count the grids are sized for.  No device code: nothing in here reaches a kernel.
#pragma once
#include <hip/hip_runtime.h>

namespace gg {

// compute units of a device, or GYMGO_AMD_CUS (gg_kernels.hip, which keeps the per-device cache); 256 when HIP cannot say
int cus_of(int dev);

// Kernels are launched on the device that OWNS the buffers (the stream handed over belongs to it too), whatever the
// calling thread's current device is; the current device is restored on return.  One hipPointerGetAttributes per call.
struct OnDeviceOf {
  int prev = -1, dev = 0;
  bool switched = false;
  explicit OnDeviceOf(const void *p) {
    (void)hipGetDevice(&prev);
    dev = prev < 0 ? 0 : prev;
    hipPointerAttribute_t at;
    if (p && hipPointerGetAttributes(&at, p) == hipSuccess) dev = at.device;
    else (void)hipGetLastError();   // a pointer HIP does not know: launch on the current device (and fail there)
    if (dev != prev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~OnDeviceOf() {
    if (switched) (void)hipSetDevice(prev);
  }
  int cus() const { return cus_of(dev); }
};

}  // namespace gg
