// Staging of the C entry points' array arguments, each of which may live in host or device memory ("Host-or-device
// arguments").  A device array is used where it lies; a host array goes through a DevBuf of the context that THE SITE NAMES: the
// buffers are shared with the kernels launched between at() and back() and with the calls nested inside, so nothing here picks one.
#pragma once
#include "fz_ctx.h"

enum StageDir { STAGE_IN = 1, STAGE_OUT = 2, STAGE_INOUT = 3 };

// Rows [i0, i0 + n) of an argument, chunk by chunk.  The pointer's kind is asked for once, here.  A NULL argument gives a NULL view,
// or with `scratch` the named buffer (an optional output that the kernel writes all the same).  Under for_row_chunks
// (fz_rows_host.inc) such a buffer counts towards the bytes per object: a call with one is chunked even when every array is on the device.
struct StageRows {
    fz_ctx* c = nullptr; char* host = nullptr; size_t row = 0; DevBuf* buf = nullptr; int dir = 0; bool dev = false, scratch = false;
    StageRows() = default;
    StageRows(fz_ctx* c_, const void* p, size_t row_bytes, DevBuf& b, int dir_, bool scratch_ = false)
        : c(c_), host((char*)p), row(row_bytes), buf(&b), dir(dir_), dev(is_device_ptr(p)), scratch(scratch_) {}
    void* cur = nullptr;                                             // the current chunk's view, where a loop keeps it (for_row_chunks)
    template <class T> T* as() const { return (T*)cur; }
    bool staged() const { return host && !dev; }
    // the device view: the array itself at row i0, or the buffer, grown and (in / inout) filled with the caller's rows
    template <class T> int at(int64_t i0, int64_t n, T** d) const {
        if (dev) { *d = (T*)(host + (size_t)i0 * row); return 0; }
        if (!host && !scratch) { *d = nullptr; return 0; }
        FZCHK(buf->ensure((size_t)n * row));
        if (host && (dir & STAGE_IN)) FZCHK(copy_in(c, buf->p, host + (size_t)i0 * row, (size_t)n * row));
        *d = (T*)buf->p;
        return 0;
    }
    // after the launch: the rows of a staged out / inout argument go back to the caller
    int back(int64_t i0, int64_t n) const {
        if (!staged() || !(dir & STAGE_OUT)) return 0;
        return copy_out(c, host + (size_t)i0 * row, buf->p, (size_t)n * row);
    }
};

// Whole arrays of one call, in the slots d_net[0..9] in the order they are asked for; finish() copies the staged outputs back.
struct StageWhole {
    fz_ctx* c; int used = 0;
    struct Out { void* host; void* dev; size_t bytes; };
    std::vector<Out> outs;
    int slot(size_t bytes, void** dev) {
        if (used >= 10) return fail(-1, "internal: staging slots exhausted");
        DevBuf& b = c->d_net[used++];
        FZCHK(b.ensure(bytes ? bytes : 8));
        *dev = b.p;
        return 0;
    }
    int in(const void* p, size_t bytes, const void** dev) {
        if (!p || is_device_ptr(p)) { *dev = p; return 0; }
        void* d;
        FZCHK(slot(bytes, &d));
        FZCHK(copy_in(c, d, p, bytes));
        *dev = d;
        return 0;
    }
    int out(void* p, size_t bytes, void** dev) {
        if (!p || is_device_ptr(p)) { *dev = p; return 0; }
        FZCHK(slot(bytes, dev));
        outs.push_back({p, *dev, bytes});
        return 0;
    }
    // out() whose staged copy starts as the caller's array: in/out arrays, and outputs only part of which is written
    int inout(void* p, size_t bytes, void** dev) {
        FZCHK(out(p, bytes, dev));
        return *dev != p ? copy_in(c, *dev, p, bytes) : 0;
    }
    int finish() {
        for (auto& o : outs) FZCHK(copy_out(c, o.host, o.dev, o.bytes));
        return 0;
    }
};

// a few values of a maybe-device array read on the host, and a host value written into a maybe-device result; complete on return
inline int host_read(void* dst, const void* src, size_t bytes) {
    if (is_device_ptr(src)) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    else std::memcpy(dst, src, bytes);
    return 0;
}
inline int host_write(void* dst, const void* src, size_t bytes) {
    if (is_device_ptr(dst)) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    else std::memcpy(dst, src, bytes);
    return 0;
}
