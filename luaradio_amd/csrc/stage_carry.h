// stage_carry.h - what a streaming stage carries from one call to the next (filter history, the previous sample, a recurrence state, pending
// bits), in two device slots that alternate.  The rule, for every stage: a call reads in(); its kernels write out(); the call flips once, behind
// its last launch, and not at all where it returns an error.  reset() puts the pair back on its first slot with both slots filled.
// (part of liblrhip.so; included by lrhip.hip right after stage.h, one translation unit.  Plain host code)
#pragma once

// A pair whose size the stage knows only at run time: two buffers of `bytes` bytes, zero after reset().
struct TwoSlots {
    DeviceBuf slot[2];
    int cur = 0;
    int reset(size_t bytes) { cur = 0; return (zero_fill(slot[0], bytes) || zero_fill(slot[1], bytes)) ? -1 : 0; }
    void *in() const { return slot[cur].p; }
    void *out() const { return slot[cur ^ 1].p; }
    template <class T> const T *in() const { return (const T *)slot[cur].p; }
    template <class T> T *out() const { return (T *)slot[cur ^ 1].p; }
    void flip() { cur ^= 1; }
};

// A pair of a fixed type: state S in two adjacent slots of one buffer, and BYTES carried bytes the same way (ci() / co()).
template <class S, int BYTES = 0> struct Carried {
    DeviceBuf state, bytes;
    int cur = 0;
    // both slots = v, the carried bytes zero
    int reset(const S &v)
    {
        cur = 0;
        S s[2];
        memcpy(&s[0], &v, sizeof(S));
        memcpy(&s[1], &v, sizeof(S));
        if (upload(state, s, sizeof(s))) return -1;
        return BYTES ? zero_fill(bytes, 2 * (size_t)BYTES) : 0;
    }
    // both slots zero
    int reset()
    {
        cur = 0;
        if (zero_fill(state, 2 * sizeof(S))) return -1;
        return BYTES ? zero_fill(bytes, 2 * (size_t)BYTES) : 0;
    }
    const S *in() const { return (const S *)state.p + cur; }
    S *out() { return (S *)state.p + (cur ^ 1); }
    const uint8_t *ci() const { return (const uint8_t *)bytes.p + (size_t)cur * BYTES; }
    uint8_t *co() { return (uint8_t *)bytes.p + (size_t)(cur ^ 1) * BYTES; }
    void flip() { cur ^= 1; }
    // The data-dependent count of the counted stages (stage_counted.h): the one small read-back of a stage, behind its last launch and flip().
    // Copies the state the call has just written into `got` and waits for the stream.  The pinned buffer exists from the first fetch() on, so a
    // stage that never reads back pins nothing.
    PinnedBuf host;
    int fetch(S &got)
    {
        if (host.reserve(sizeof(S))) return -1;
        LR_HIP(hipMemcpyAsync(host.p, in(), sizeof(S), hipMemcpyDeviceToHost, ctx().stream));
        LR_HIP(hipStreamSynchronize(ctx().stream));
        got = *(const S *)host.p;
        return 0;
    }
};
