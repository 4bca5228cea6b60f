// The account table's handle, shared by the engine entries (capi_engine.cpp) and the drop-in entries (capi_zk.cpp).  The table locks for itself (its own mutex, then
// the device mutex: gpu_accounts.hip), so its entries do not take the device mutex.
#pragma once
#include "gpu.hpp"

struct zkgpu_accts { zk::AccountTable a; zkgpu_accts(int log2_slots, const uint64_t *seed) : a(log2_slots, seed) {} };
