// The bookkeeping of a host-form call's staging image (no other header of the library needed and no HIP:
// tests/cpp/stage_check.cpp compiles this file alone).
//
// A call describes what it stages ONCE, as a callable over a Stage: a sequence of pieces, each starting on a 256-byte
// boundary of one image that exists twice, in pinned host memory (h) and in device memory (d).  The callable runs twice:
//   - stage_measure runs it on a Stage without buffers.  Pieces only advance the offset; no filler is invoked and the
//     addresses it hands out are not to be used.  The end offset is what the buffers have to hold.
//   - the caller then runs it on the Stage whose h and d it sized from that figure.  Every filler runs once, with the
//     host address of its piece, and the piece's device address is what the kernels get.
// Both passes see the same statements, so the sizes cannot disagree with what is staged.  The callable must therefore
// be repeatable: it assigns device addresses and stages, nothing else.
//
// Pieces that travel back are recorded (back / out / inout): after the launch the caller fetches the span from the first
// recorded piece to the end of the last in one copy and scatter() hands each recorded piece to its host array.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace orbhip {

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

struct Stage {
    enum { kMaxOut = 24 };                // recorded pieces of one call (most today: 17, orbhip_cull_key_frames)
    struct Out { void *host; size_t off, bytes; };

    uint8_t *h = nullptr, *d = nullptr;   // the image in pinned and in device memory; both null in the measuring pass
    size_t off = 0;                       // end of the last piece, a multiple of 256
    Out outs[kMaxOut];
    int n_out = 0;
    bool out_overflow = false;            // a record beyond kMaxOut was refused: the caller fails the call
    const uint8_t *img = nullptr;         // the fetched span [out_begin(), out_end()), set by the caller after its copy

    // room for `count` T that nothing fills here: the device address of the piece.  A piece of no elements takes no
    // room and yields the address of the piece after it.
    template <class T> T *room(size_t count)
    {
        T *dev = reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(d) + off);
        off += al256(count * sizeof(T));
        return dev;
    }
    // room for `count` T that filler(T *host) writes in place (real pass only, and only for count > 0)
    template <class T, class F> T *fill(size_t count, F &&filler)
    {
        const size_t at = off;
        T *dev = room<T>(count);
        if (h && count) filler(reinterpret_cast<T *>(h + at));
        return dev;
    }
    // several pieces that one loop fills (the rows of a bank): room() for each, then sweep(filler).  The filler runs in
    // the real pass only and gets the host address of a piece from host(dev).
    template <class F> void sweep(F &&filler) { if (h) filler(); }
    template <class T> T *host(const T *dev) const { return reinterpret_cast<T *>(h + (reinterpret_cast<uintptr_t>(dev) - reinterpret_cast<uintptr_t>(d))); }
    template <class T> const T *put(const T *src, size_t count)   // a copy of src[0 .. count): an input, read-only on the device
    {
        return fill<T>(count, [=](T *host) { memcpy(host, src, count * sizeof(T)); });
    }
    // the piece of `count` T at device address dev travels back, to host[0 .. count) (null: it is only part of the
    // fetched span, for image()).  An empty piece is not recorded.
    template <class T> void back(T *host, const T *dev, size_t count)
    {
        if (!count) return;
        if (n_out == kMaxOut) { out_overflow = true; return; }
        outs[n_out++] = Out{host, (size_t)(reinterpret_cast<uintptr_t>(dev) - reinterpret_cast<uintptr_t>(d)), count * sizeof(T)};
    }
    template <class T> T *out(T *host, size_t count)     // room that the kernels fill, copied to host afterwards
    {
        T *dev = room<T>(count);
        back(host, dev, count);
        return dev;
    }
    template <class T> T *inout(T *host, size_t count)   // staged from host, copied back to it afterwards
    {
        T *dev = fill<T>(count, [=](T *image) { memcpy(image, host, count * sizeof(T)); });
        back(host, dev, count);
        return dev;
    }

    // the span to fetch; pieces are recorded as they are staged, so the records ascend
    size_t out_begin() const { return n_out ? outs[0].off : off; }
    size_t out_end() const { return n_out ? outs[n_out - 1].off + outs[n_out - 1].bytes : off; }
    // each recorded piece of the fetched span to its host array, and nothing else
    void scatter(const uint8_t *fetched)
    {
        img = fetched;
        const size_t b = out_begin();
        for (int i = 0; i < n_out; ++i)
            if (outs[i].host) memcpy(outs[i].host, fetched + (outs[i].off - b), outs[i].bytes);
    }
    // where the fetched span holds the piece at device address dev
    template <class T> const T *image(const T *dev) const
    {
        return reinterpret_cast<const T *>(img + (reinterpret_cast<uintptr_t>(dev) - reinterpret_cast<uintptr_t>(d) - out_begin()));
    }
};

// the bytes `pieces` stages: its end offset on a Stage without buffers
template <class F> size_t stage_measure(F &&pieces, bool *out_overflow = nullptr)
{
    Stage measure;
    pieces(measure);
    if (out_overflow) *out_overflow = measure.out_overflow;
    return measure.off;
}

}   // namespace orbhip
