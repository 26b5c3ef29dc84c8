// The part of the C ABI (include/segdino3d_hip.h) that belongs to no kernel file: error text, ABI version, host self-test.
// Every other sd3d_* entry point is defined in the file that owns its kernels.
#include "common.h"
#include "../../include/segdino3d_hip.h"
#include <string.h>
#include <stdio.h>

static thread_local char g_err[512] = "";

int sd3d_set_error(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg ? msg : "unknown error");
    return code;
}

extern "C" {

int sd3d_abi_version(void) { return SD3D_ABI_VERSION; }
const char* sd3d_last_error(void) { return g_err; }

int sd3d_selftest_host(void) {
    // Z-order codec round trip + parent relation (runs on the host, no GPU needed)
    uint32_t s = 12345u;
    for (int it = 0; it < 20000; ++it) {
        s = s * 1664525u + 1013904223u; const uint32_t x = (s >> 8) & 0xFFFF;
        s = s * 1664525u + 1013904223u; const uint32_t y = (s >> 8) & 0xFFFF;
        s = s * 1664525u + 1013904223u; const uint32_t z = (s >> 8) & 0xFFFF;
        const uint64_t m = morton_encode(x, y, z);
        uint32_t a, b, c;
        morton_decode(m, a, b, c);
        if (a != x || b != y || c != z) return sd3d_set_error(-100, "morton round trip failed");
        if ((m >> 3) != morton_encode(x >> 1, y >> 1, z >> 1)) return sd3d_set_error(-101, "morton parent relation failed");
        if ((m & 7ull) != ((x & 1) | ((y & 1) << 1) | ((z & 1) << 2))) return sd3d_set_error(-102, "morton child bits failed");
        if (m >> 48) return sd3d_set_error(-103, "morton exceeds 48 bits");
    }
    return 0;
}

}  // extern "C"
