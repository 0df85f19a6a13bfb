// Library core: version string, thread-local error message, launch check, test-hook state and environment switches.
#include "internal.h"

static thread_local char g_err[512] = "";

int pcrl_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int pcrl_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pcrl_fail(PCRL_ELAUNCH, "%s: launch failed: %s", what, hipGetErrorString(e));
  return PCRL_OK;
}

extern "C" const char* pcrl_version(void) { return "pcrl_hip 0.1 (gfx950)"; }
extern "C" const char* pcrl_last_error(void) { return g_err; }

// Zero-fill of a device buffer on the caller's stream (the runtime's fill: no kernel of ours, none of ATen's) -- e.g. dx of a 1x1 stride-2
// convolution's data gradient, three of whose four parity classes receive nothing (pcrl_conv2d_dgrad_s2).
extern "C" int pcrl_zero(void* p, size_t bytes, pcrl_stream_t stream) {
  PCRL_REQUIRE(p && bytes > 0, "zero: bad arguments");
  const hipError_t e = hipMemsetAsync(p, 0, bytes, as_stream(stream));
  if (e != hipSuccess) return pcrl_fail(PCRL_ELAUNCH, "zero: hipMemsetAsync failed: %s", hipGetErrorString(e));
  return PCRL_OK;
}

// ---- test hooks (pcrl_hip.h: "Test hooks"): the code tables, written once ----------------------------------------------------------
PcrlHooks g_hooks;

//   impl of pcrl_debug_set_conv_impl              conv_impl  brick_ymap  brick16_on  brick16_planes
//   0  auto                                            0          1           1           -1
//   1  gather kernel                                   1          1           0           -1
//   2  gather kernel without split-K                   2          1           0           -1
//   3  4x8x8-brick kernel on its plain 2-D grid        0          0           0           -1
//   4  4x8x8-brick kernel wherever it is eligible      0          1           0           -1
//   5  auto, wide brick on 4-plane bricks only         0          1           1            0
//   6  auto, wide brick on 8-plane bricks if they tile 0          1           1            2
extern "C" void pcrl_debug_set_conv_impl(int impl) {
  g_hooks.conv_impl = (impl >= 3 && impl <= 6) ? 0 : impl;
  g_hooks.brick_ymap = impl != 3;
  g_hooks.brick16_on = impl == 0 || impl == 5 || impl == 6;
  g_hooks.brick16_planes = impl == 5 ? 0 : impl == 6 ? 2 : -1;
}
//   impl of pcrl_debug_set_wgrad_impl             wgrad_impl  wb_xcd  wb_order  wb_tiles
//   0  auto                                            0          1        1         1
//   1  gather kernel                                   1          0        0         1
//   2  brick kernel, plain 2-D grid, old walk order    0          0        0         1
//   4  brick kernel, co-located, old walk order        0          1        0         1
//   5  brick kernel, plain 2-D grid, new walk order    0          0        1         1
//   6  brick kernel, co-located, 64 x 64 tiles only    0          1        1         0
extern "C" void pcrl_debug_set_wgrad_impl(int impl) {
  g_hooks.wgrad_impl = impl == 1 ? 1 : 0;
  g_hooks.wb_xcd = impl == 0 || impl == 4 || impl == 6;
  g_hooks.wb_order = impl == 0 || impl == 5 || impl == 6;
  g_hooks.wb_tiles = impl != 6;
}
extern "C" void pcrl_debug_set_wgrad_tr(int on) { g_hooks.wgrad_tr = on; }
// conv2d impl: 0 auto, 1 always the gather kernel, 2 auto without the wide brick
extern "C" void pcrl_debug_set_conv2d_impl(int impl) { g_hooks.conv2d_impl = impl; }
extern "C" void pcrl_debug_set_reduce_repeat(int n) { g_hooks.reduce_repeat = n < 1 ? 1 : n; }

const PcrlEnv& pcrl_env() {
  static const PcrlEnv env = [] {
    const char *b = getenv("PCRL_DGRAD_BNRED"), *v = getenv("PCRL_IGEMM_VMAJOR"), *t = getenv("PCRL_UPC_PACK_TILED");
    return PcrlEnv{b && b[0] == '0', v ? atoi(v) == 1 ? 8 : atoi(v) : 8, !(t && t[0] == '0')};
  }();
  return env;
}
