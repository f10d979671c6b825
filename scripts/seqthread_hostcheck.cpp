// seqthread_hostcheck.cpp — a stand-alone program (its own main, no Python) over the host-side argument checks of the threading entry
// points (aix_seqthread.hip): every refusal that is decided before anything is allocated or launched, so it runs without a GPU. Meant for
// a host sanitizer build of that one translation unit, linked in front of the library, which supplies everything else:
//   hipcc -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -c aindex_amd/csrc/aix_seqthread.hip -o st.o
//   clang++ -O1 -g -std=c++17 -Iinclude -fsanitize=address,undefined -c scripts/seqthread_hostcheck.cpp -o main.o
//   hipcc --hip-link --offload-arch=gfx950 -fsanitize=address,undefined main.o st.o aindex_amd/lib/libaindex_hip.so -o hostcheck && ./hostcheck
// (scripts/host_sanitize.sh runs the CPU suite against a sanitized library and does not take a program.) Exit status = violations found.
#include <cstdint>
#include <cstdio>

#include "aindex_hip.h"

int main() {
    uint64_t a[4] = {0, 0, 0, 0}, tot = 77;
    void* p = a;
    int bad = 0;
    bad += aix_graph_kidmap_dev(1, nullptr, (uint32_t*)p, (uint8_t*)p, 1, a, (uint32_t*)p, a, (uint8_t*)p, a, (uint32_t*)p, (uint8_t*)p, nullptr) != AIX_ERR_ARG;
    bad += aix_graph_kidmap_dev(1, a, (uint32_t*)p, (uint8_t*)p, 1, nullptr, (uint32_t*)p, a, (uint8_t*)p, a, (uint32_t*)p, (uint8_t*)p, nullptr) != AIX_ERR_ARG;
    bad += aix_graph_kidmap_dev(0, nullptr, nullptr, nullptr, 0, a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != AIX_OK;
    bad += aix_thread_nodes_dev(1, a, (uint32_t*)p, (uint8_t*)p, 1, a, nullptr, nullptr) != AIX_ERR_ARG;
    bad += aix_thread_nodes_dev(1, a, (uint32_t*)p, (uint8_t*)p, (1ull << 31) - 3, a, a, nullptr) != AIX_ERR_UNSUPPORTED;
    bad += aix_thread_nodes_dev(0, nullptr, nullptr, nullptr, 0, a, nullptr, nullptr) != AIX_OK;
    bad += aix_seq_thread_dev(nullptr, nullptr, a, 1, a, 1, a, (uint8_t*)p, a, (uint32_t*)p, 0, nullptr, a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &tot, nullptr) != AIX_ERR_ARG;
    bad += aix_seq_thread(nullptr, 0, nullptr, a, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != AIX_ERR_ARG;
    bad += tot != 77;
    printf("violations %d\n", bad);
    return bad;
}
