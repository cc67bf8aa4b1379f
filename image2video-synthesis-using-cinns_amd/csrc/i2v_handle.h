// The handle layer of libi2v_hip.so: what every i2v_* handle type shares -- creation, load, the prologue of a call that enqueues
// work, and the workspace layout arithmetic.  A handle struct has `int device` (the device its packed weights live on) and
// `bool loaded`; the types whose calls are serialised across streams also hold a StreamOrder ("Handles", lists them).
#pragma once
#include <memory>

#include "i2v_common.h"

namespace i2v {

// *_create, behind the type's own argument checks: a device must exist; the handle is allocated and bound to the current device;
// init(H*) does the type-specific part and may refuse (its code is returned and the handle freed); *out is written on success only.
template <class H, class Init>
int create_handle(const char* what, H** out, Init init) {
    I2V_REQUIRE(out, I2V_E_INVALID, "%s: null argument", what);
    int ndev = 0;
    I2V_HIP_CHECK(hipGetDeviceCount(&ndev));
    I2V_REQUIRE(ndev > 0, I2V_E_HIP, "%s: no HIP device", what);
    auto h = std::make_unique<H>();
    I2V_HIP_CHECK(hipGetDevice(&h->device));
    if (int rc = init(h.get())) return rc;
    *out = h.release();
    return I2V_OK;
}

// *_load: pack(h, state_dict) repacks and uploads the weights.  The handle is UNLOADED while it runs and stays so unless it returns
// I2V_OK: a load that fails half-way (a missing key) leaves a mixture of old and new packed weights behind, and the next call that
// needs weights answers I2V_E_STATE instead of running on it.  The only place that writes `loaded`.
template <class H>
int load_handle(const char* what, H* h, const i2v_tensor* tensors, int n_tensors, int (*pack)(H*, const StateDict&)) {
    I2V_REQUIRE(h, I2V_E_INVALID, "%s: null argument", what);
    I2V_REQUIRE_DEVICE(h->device, what);
    I2V_REQUIRE(tensors && n_tensors > 0, I2V_E_INVALID, "%s: null argument", what);
    h->loaded = false;
    const StateDict sd(tensors, n_tensors);
    const int rc = pack(h, sd);
    h->loaded = rc == I2V_OK;
    return rc;
}

// The scope of a call that enqueues work on a handle.  check() first: the handle, its device, its weights.  The entry's own
// argument and workspace checks follow, then -- for a type with a StreamOrder -- serialise(): a call that arrives on another
// stream than the previous one waits for it, and the end of this call is recorded on its stream when the scope is left, on the
// error paths too (whatever was enqueued is ordered).  Neither step makes a HIP call the entries did not make before they shared
// this code: one hipGetDevice, and StreamOrder's own calls only where the type has one.
struct Entry {
    enum : unsigned {
        NEEDS_WEIGHTS = 1,      // I2V_E_STATE unless the handle is loaded
        NULL_IS_UNLOADED = 2,   // a null handle answers I2V_E_STATE, not I2V_E_INVALID: the whole-network forwards have always
                                // reported it as "weights not loaded", and callers may compare the code
    };
    StreamOrder* order = nullptr;
    hipStream_t st = nullptr;
    Entry() = default;
    Entry(const Entry&) = delete;
    Entry& operator=(const Entry&) = delete;
    ~Entry() { if (order) order->exit(st); }

    template <class H>
    int check(const H* h, unsigned flags, const char* what) {
        if (flags & NULL_IS_UNLOADED) I2V_REQUIRE(h, I2V_E_STATE, "%s: weights not loaded", what);
        I2V_REQUIRE(h, I2V_E_INVALID, "%s: null handle", what);
        I2V_REQUIRE_DEVICE(h->device, what);
        I2V_REQUIRE(!(flags & NEEDS_WEIGHTS) || h->loaded, I2V_E_STATE, "%s: weights not loaded", what);
        return I2V_OK;
    }
    int serialise(StreamOrder& o, hipStream_t s) {
        if (int rc = o.entry(s)) return rc;
        order = &o; st = s;
        return I2V_OK;
    }
};
// declares the scope `sc` and runs its check
#define I2V_ENTER(sc, h, flags, what) \
    i2v::Entry sc;                    \
    if (int rc_enter_ = sc.check(h, flags, what)) return rc_enter_

#define I2V_REQUIRE_WORKSPACE(have, need, what) \
    I2V_REQUIRE((have) >= (need), I2V_E_WORKSPACE, "%s: workspace %zu < required %zu", what, (size_t)(have), (size_t)(need))

// A launch plan built on the host (i2v_trunk_plan.h) that refused its shape: its message and code become the call's
template <class Plan>
int plan_refusal(const Plan& p) {
    set_error("%s", p.error);
    return p.status;
}

// Carves a workspace into slots: every take returns the slot's byte offset, and the next slot starts 256-byte aligned behind it
// (a zero-sized slot takes no room and shares its offset with the next one).
struct Carver {
    size_t o = 0;
    size_t take_bytes(size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; }
    size_t take_floats(size_t floats) { return take_bytes(floats * 4); }
    size_t total() const { return o; }
    template <class T = float>
    static T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
};

}  // namespace i2v
