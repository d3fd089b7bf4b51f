// Who owns device and pinned memory, and what an allocation that fails leaves behind: nothing.
//
// Host-only and free of HIP headers: everything is templated on a backend B, so that a plain C++ program can run
// it over malloc (tests/mem_owner_main.cpp).  B supplies
//     typedef ... error;  static constexpr error ok;
//     static error alloc(void **p, size_t bytes);          static void free(void *p);
//     static error alloc_pinned(void **p, size_t bytes);   static void free_pinned(void *p);
//     error fill(void *p, int byte, size_t bytes);         error copy(void *dst, const void *src, size_t bytes);
//     error sync();                                        // fill and copy may be asynchronous: wait for them
//
// Everything here, the HIP backend (tspgpu_hipmem.h) and the structs of the engine built from them have hidden visibility:
// libtspgpu.so exports its C ABI (include/tspgpu.h) and none of the weak instantiations of these templates.
#pragma once
#include <cstddef>
#include <initializer_list>
#include <utility>
#include <vector>

namespace tspmem __attribute__((visibility("hidden"))) {

template <class B> void release(void *p, bool pinned) { if (p) { if (pinned) B::free_pinned(p); else B::free(p); } }

template <class T> struct elem_bytes { static constexpr size_t value = sizeof(T); };
template <> struct elem_bytes<void> { static constexpr size_t value = 1; };     // a Buf<void> counts bytes

// Move-only owner of `n` elements at `p`.  It converts to the raw pointer, which is what kernels and copies take.
template <class B, class T, bool PINNED> struct Buf {
    T *p = nullptr;
    size_t n = 0;

    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    Buf &operator=(Buf &&o) noexcept { if (this != &o) { reset(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
    ~Buf() { reset(); }
    operator T *() const { return p; }

    void reset() { release<B>(p, PINNED); p = nullptr; n = 0; }
    // `count` elements, contents undefined; what was held goes first.  On failure the buffer is empty.
    typename B::error alloc(size_t count)
    {
        reset();
        void *q = nullptr;
        const size_t bytes = count * elem_bytes<T>::value;
        const typename B::error e = PINNED ? B::alloc_pinned(&q, bytes) : B::alloc(&q, bytes);
        if (e == B::ok) { p = static_cast<T *>(q); n = count; }
        return e;
    }
    // grow-only: room for `count` elements.  Growing does not keep the contents.
    typename B::error reserve(size_t count) { return count <= n ? B::ok : alloc(count); }
};
template <class B, class T> using DevBuf = Buf<B, T, false>;
template <class B, class T> using PinBuf = Buf<B, T, true>;

template <class... Bufs> void reset_all(Bufs &...b) { (b.reset(), ...); }

// alloc_all<B>({{&a, na}, {&b, nb}, ...}): every buffer listed, or none -- after a failure all of them are empty
template <class B> struct Want {
    void *buf; size_t count;
    typename B::error (*alloc)(void *, size_t);
    void (*reset)(void *);
    template <class T, bool P> Want(Buf<B, T, P> *b, size_t c)
        : buf(b), count(c), alloc([](void *q, size_t k) { return static_cast<Buf<B, T, P> *>(q)->alloc(k); }),
          reset([](void *q) { static_cast<Buf<B, T, P> *>(q)->reset(); }) {}
};
template <class B> typename B::error alloc_all(std::initializer_list<Want<B>> want)
{
    typename B::error e = B::ok;
    for (const Want<B> &w : want) if ((e = w.alloc(w.buf, w.count)) != B::ok) break;
    if (e != B::ok) for (const Want<B> &w : want) w.reset(w.buf);
    return e;
}

// One array of a struct of raw pointers that kernels take by value (a view): `slot` is the view's field, the array holds
// units * unit_bytes + slack_bytes.  A row with unit_bytes == 0 has one size whatever the units: it is allocated once
// and kept while it is held.
struct Row {
    static constexpr int NO_FILL = -1;
    void **slot; size_t unit_bytes, slack_bytes; int fill; bool keep_old, pinned;
    template <class T> Row(T **s, size_t unit, size_t slack = 0, int fill_byte = NO_FILL, bool keep = false, bool pin = false)
        : slot(reinterpret_cast<void **>(s)), unit_bytes(unit), slack_bytes(slack), fill(fill_byte), keep_old(keep), pinned(pin) {}
    size_t bytes(size_t units) const { return units * unit_bytes + slack_bytes; }
    bool held_once() const { return unit_bytes == 0 && *slot; }
};
typedef std::vector<Row> Rows;

inline size_t rows_bytes(const Rows &rows, size_t units)
{
    size_t total = 0;
    for (const Row &r : rows) total += r.bytes(units);
    return total;
}

template <class B> void free_rows(const Rows &rows)
{
    for (const Row &r : rows) { release<B>(*r.slot, r.pinned); *r.slot = nullptr; }
}

// The arrays of `rows` from old_units to new_units, all or none: allocate every new array, fill it, copy the first
// old_units of the rows that keep them, wait; only then free the old arrays and write the new pointers into the view.
// On any failure the new arrays are freed and the view, with what it points to, is as before the call.
template <class B> typename B::error grow(B b, const Rows &rows, size_t old_units, size_t new_units)
{
    std::vector<void *> fresh(rows.size(), nullptr);
    typename B::error e = B::ok;
    bool filled = false, copied = false;
    for (size_t k = 0; k < rows.size() && e == B::ok; k++) {
        const Row &r = rows[k];
        if (r.held_once()) continue;
        e = r.pinned ? B::alloc_pinned(&fresh[k], r.bytes(new_units)) : B::alloc(&fresh[k], r.bytes(new_units));
    }
    for (size_t k = 0; k < rows.size() && e == B::ok; k++)
        if (fresh[k] && rows[k].fill != Row::NO_FILL) {
            e = b.fill(fresh[k], rows[k].fill, rows[k].bytes(new_units));
            filled = true;
        }
    for (size_t k = 0; k < rows.size() && e == B::ok; k++)
        if (fresh[k] && rows[k].keep_old && old_units && *rows[k].slot) {
            e = b.copy(fresh[k], *rows[k].slot, old_units * rows[k].unit_bytes);
            copied = true;
        }
    if (e == B::ok && copied) e = b.sync();
    if (e != B::ok) {
        if (filled || copied) b.sync();     // nothing may still write into what is freed
        for (size_t k = 0; k < rows.size(); k++) release<B>(fresh[k], rows[k].pinned);
        return e;
    }
    for (size_t k = 0; k < rows.size(); k++) {
        const Row &r = rows[k];
        if (r.held_once()) continue;
        release<B>(*r.slot, r.pinned);
        *r.slot = fresh[k];
    }
    return B::ok;
}

} // namespace tspmem
