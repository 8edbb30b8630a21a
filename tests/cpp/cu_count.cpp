// Prints device 0's compute-unit count as mcc_create reads it (hipDeviceGetAttribute, 256 when the
// query fails): tests that run the host-only planner for a live problem pass it as n_cu / n_cu_dev.
#include <cstdio>

#include <hip/hip_runtime_api.h>

int main() {
    int n = 256;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess || n <= 0) n = 256;
    std::printf("%d\n", n);
    return 0;
}
