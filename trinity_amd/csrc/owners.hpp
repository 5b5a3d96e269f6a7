// owners.hpp — who releases what.  One move-only owning handle per way the host runtime obtains device memory, pinned memory, an event or a reference
// on the device handle; a member or a local of one of these types is released when it goes out of scope or is assigned anew, so no destructor and no
// error path lists its buffers by hand.  The TYPE names the allocator — it cannot be released through the wrong call:
//   DevMem<T>     hipMalloc / hipFree (hipFree synchronises the device: the index's columns, per-call decode temporaries, the collection's blocks)
//   Pooled<T>     pool_alloc / pool_free of the device handle's pool (no device call once the pool is warm)
//   Pinned<T>     pinned_alloc / pinned_free: a pinned host block and its capacity
//   PooledEvent   event_get / event_put
//   DevRef        dev_retain / dev_release: declared FIRST in an object, so that it is released after every buffer of the object
// Each is a std::unique_ptr (empty by default; reset(), release(), get(), move) that also converts to its plain pointer, so kernel arguments, pointer
// arithmetic and casts read as they do for a raw pointer; a pointer INTO a buffer (an arena section, a row of a block) stays a plain pointer: a view.
// No lock, allocation or bookkeeping beyond what the calls themselves do.  Included by trinity_hip.hip behind the pool's functions (the same translation unit).
#pragma once
#include <memory>
#include <type_traits>

template <class T, class Free> // Free: the release call, and what it needs beside the pointer
struct Owner : std::unique_ptr<T, Free> {
        using std::unique_ptr<T, Free>::unique_ptr;
        operator T *() const { return this->get(); }
};

struct FreeDevice {
        void operator()(void *q) const { hipFree(q); }
};
struct FreePooled {
        tri_dev *dev = nullptr;
        void operator()(void *q) const { pool_free(dev, q); }
};
struct FreePinned {
        tri_dev *dev = nullptr;
        size_t cap = 0; // the block's size as the pool knows it
        void operator()(void *q) const { pinned_free(dev, q, cap); }
};
struct PutEvent {
        tri_dev *dev = nullptr;
        void operator()(hipEvent_t e) const { event_put(dev, e); }
};
struct DropRef {
        void operator()(tri_dev *d) const { dev_release(d); }
};

template <class T>
struct DevMem : Owner<T, FreeDevice> {
        hipError_t alloc(const size_t bytes) { // (what it held is released first)
                this->reset();
                void *q = nullptr;
                const hipError_t e = hipMalloc(&q, bytes);
                this->reset(static_cast<T *>(q));
                return e;
        }
};
template <class T>
struct Pooled : Owner<T, FreePooled> {
        using Owner<T, FreePooled>::Owner; // (Pooled(p, FreePooled{dev}) adopts a pool_alloc'ed buffer)
        hipError_t alloc(tri_dev *d, const size_t bytes) {
                this->reset();
                this->get_deleter().dev = d;
                void *q = nullptr;
                const hipError_t e = pool_alloc(d, &q, bytes);
                this->reset(static_cast<T *>(q));
                return e;
        }
};
template <class T>
struct Pinned : Owner<T, FreePinned> {
        T *alloc(tri_dev *d, const size_t bytes) { // nullptr: no pinned memory to be had
                this->reset();
                this->get_deleter().dev = d;
                this->reset(reinterpret_cast<T *>(pinned_alloc(d, bytes, &this->get_deleter().cap)));
                return this->get();
        }
};
struct PooledEvent : Owner<std::remove_pointer_t<hipEvent_t>, PutEvent> {
        hipError_t take(tri_dev *d) {
                reset();
                get_deleter().dev = d;
                hipEvent_t e = nullptr;
                const hipError_t rc = event_get(d, &e);
                reset(e);
                return rc;
        }
};
struct DevRef : Owner<tri_dev, DropRef> {
        void retain(tri_dev *d) {
                dev_retain(d);
                reset(d);
        }
};
