// What every extern "C" entry of libgoi_raster.so refuses a call with (host only).  Defined once, in api.hip, over the one
// thread_local message that goi_raster_last_error returns.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

namespace goi {

int fail(const char* where, hipError_t e);  // "<where>: <the HIP error's text>"
int fail(const std::string& msg);

// The one refusal of a caller's workspace, for every entry: NULL, or not 256-byte aligned (the layouts carve from a 256-byte
// aligned base: workspace.h).  `what` is the argument's name in the message.
int check_workspace(const std::string& fn, const void* ws, const char* what = "workspace");

// the image size of a packed mask (masks.hip) and of the frame composed over one (display.hip)
inline int mask_dims(const char* fn, int H, int W) {
    if (H < 1 || W < 1) return fail(std::string(fn) + ": need H >= 1 and W >= 1");
    if ((long long)H * W >= (1ll << 31)) return fail(std::string(fn) + ": need H * W < 2^31");
    return 0;
}

// the sizes of a mesh, min_each <= V, F (mesh.hip; the texture bake's entries take a mesh too)
int mesh_sizes(const char* fn, long long V, long long F, long long min_each);

#define GOI_HIP(call)                                      \
    do {                                                    \
        hipError_t e__ = (call);                            \
        if (e__ != hipSuccess) return fail(#call, e__);     \
    } while (0)

}  // namespace goi
