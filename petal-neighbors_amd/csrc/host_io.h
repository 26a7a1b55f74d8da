// How a host entry point lays out its staging buffer.  A host entry copies its inputs into HBM, runs on the device and
// copies its outputs back; all of these arrays are slots of ONE allocation.  A call declares its slots in order, each an
// element size and a count, and this is the one place that decides where they lie.  Host arithmetic only (no HIP): the
// stager (HostIo, index.hip) carves with it, and tests/cpp/host_io.cpp asks it "where would these slots lie?" on the CPU.
#pragma once

#include <cstddef>

namespace pn {

constexpr size_t kIoSlots = 8;   // slots per call (pn_linkage_* declares eight, pn_kmeans_* seven)
constexpr size_t kIoAlign = 16;  // every slot starts at a multiple of this: no slot's type needs more

// Slot i is bytes [off[i], off[i] + bytes[i]) of the buffer; off[i] is the end of slot i - 1 rounded up to kIoAlign
// (slot 0: 0), a count of 0 is a slot of no bytes, and `total` -- what the buffer must hold -- is the end of the last
// slot.  A product or a sum that does not fit size_t, or a slot beyond kIoSlots, clears `ok` for good: add() then
// returns kIoSlots, and nothing of the layout may be used.
struct IoLayout {
    size_t off[kIoSlots] = {}, bytes[kIoSlots] = {};
    size_t slots = 0, total = 0;
    bool ok = true;
    size_t add(size_t elem_bytes, size_t count) {
        constexpr size_t max = ~(size_t)0;
        const size_t pad = (kIoAlign - total % kIoAlign) % kIoAlign;
        if (!ok || slots == kIoSlots || (count && elem_bytes > max / count) || pad > max - total ||
            elem_bytes * count > max - total - pad) {
            ok = false;
            return kIoSlots;
        }
        off[slots] = total + pad;
        bytes[slots] = elem_bytes * count;
        total = off[slots] + bytes[slots];
        return slots++;
    }
};

}  // namespace pn
