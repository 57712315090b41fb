// mh_domains (include/mythril_hip.h "finite domains"): per group column an interval or a value
// list, made by the analysis or the constructor in domains.cpp (host only).  The enumerating
// generator (capi.cpp mh_assign_enumerate, enumerate.hip) uploads the packed descriptors on first
// use and parks the device block here, with the routine that releases it: domains.cpp itself never
// touches a device.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/mythril_hip.h"

struct mh_domains {
    std::vector<uint32_t> cols;       // ascending
    std::vector<uint32_t> kind;       // MH_DOMAIN_*
    std::vector<uint64_t> size;       // saturating at 2^64 - 1
    std::vector<uint32_t> lo;         // [n][8], zero for a list
    std::vector<uint32_t> list_off;   // [n + 1] ranges of list_vals, in values
    std::vector<uint32_t> list_vals;  // x 8 limbs, ascending per column
    uint64_t rows = 0;                // product of the sizes, saturating
    // the device copy (made by mh_assign_enumerate for the context `dev_owner`)
    void* dev = nullptr;
    void* dev_owner = nullptr;
    void (*dev_release)(mh_domains*) = nullptr;
};
