// Error reporting shared by every entry point of libynet_hip.so (see include/ynet_hip.h).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include <atomic>

static thread_local char g_err[512] = "";

void ynet_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int ynet_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ynet_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return 2;
    }
    return 0;
}

// What the dispatchers of ynet_conv2d (slot 0) and ynet_conv2d_wgrad (slot 1) launched last (include/ynet_hip.h: ynet_conv2d_last_launch): the
// launchers note it, a reader takes it and leaves 0.  One record per process, not per thread: autograd runs a backward pass on a thread of its own.
static std::atomic<int> g_launch[2];

void ynet_note_launch(int which, int code) { g_launch[which & 1].store(code, std::memory_order_relaxed); }

extern "C" int ynet_conv2d_last_launch(int which) { return g_launch[which & 1].exchange(0, std::memory_order_relaxed); }

extern "C" const char* ynet_last_error(void) { return g_err; }
extern "C" int ynet_abi_version(void) { return 1; }
