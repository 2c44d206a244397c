// The device-free part that the slot pipelines share (dl_slot_async.cpp, ul_slot_async.cpp): the life cycle of a pool's slots
//
//   FREE --claim--> OPEN --arm--> FINISHING --complete (a runtime thread) or fail_armed--> DONE --release--> FREE
//                     `----------------------------- release ------------------------------------------------^
//
// and the locks and the condition variable it runs under, while a DU drives a pool from several threads and threads of the HIP
// runtime call back into it.  Needs the public header alone (tests/slot_pool_check.cpp compiles it by itself, also under the
// thread sanitizer).  Not part of the ABI.
#pragma once

#include "mi355_nrphy.h"

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <vector>

#pragma GCC visibility push(hidden)

enum class SlotLife : uint32_t { FREE = 0, OPEN, FINISHING, DONE };

// nrphy_dl_slot_done_fn and nrphy_ul_slot_done_fn: the same signature.
typedef void (*slot_done_fn)(void* user, int status, uint32_t slot_id);

// What a slot of either pipeline starts with.  `state` is written with release and read with acquire: whoever sees DONE sees
// `status`, and whoever sees OPEN sees the slot reset.
struct SlotCore {
  uint32_t              id = 0;
  std::mutex            mutex; // serialises the calls on this slot
  std::atomic<SlotLife> state{SlotLife::FREE};
  std::atomic<int>      status{NRPHY_OK};
  slot_done_fn          done = nullptr;
  void*                 user = nullptr;
};

// What a pool of either pipeline starts with; Slot derives from SlotCore.  `mutex` guards nof_open and every change to or from
// FREE, and `changed` is notified after every change that somebody may wait for.
template <class Slot>
struct SlotPool {
  std::vector<Slot>       slots;
  std::mutex              mutex; // open / close
  std::condition_variable changed;
  uint32_t                nof_open = 0;
};

// The slot of an id handed out by slot_pool_claim and not released since; nullptr for any other id and for no pool.
template <class Slot>
Slot* slot_pool_lookup(SlotPool<Slot>* pool, uint32_t slot_id)
{
  if (pool == nullptr || slot_id >= pool->slots.size()) {
    return nullptr;
  }
  Slot* s = &pool->slots[slot_id];
  return s->state.load(std::memory_order_acquire) == SlotLife::FREE ? nullptr : s;
}

// The first free slot, now OPEN with status OK and no handler, or nullptr when all are open.  No two callers get the same slot.
template <class Slot>
Slot* slot_pool_claim(SlotPool<Slot>& pool)
{
  std::lock_guard<std::mutex> lock(pool.mutex);
  for (Slot& s : pool.slots) {
    if (s.state.load(std::memory_order_acquire) == SlotLife::FREE) {
      s.done = nullptr;
      s.user = nullptr;
      s.status.store(NRPHY_OK, std::memory_order_relaxed);
      s.state.store(SlotLife::OPEN, std::memory_order_release);
      ++pool.nof_open;
      return &s;
    }
  }
  return nullptr;
}

// Gives a claimed slot back and wakes slot_pool_wait_free.  Nothing of the slot may be in flight: after an armed slot, call
// slot_pool_await_callback first.
template <class Slot>
void slot_pool_release(SlotPool<Slot>& pool, SlotCore& s)
{
  {
    std::lock_guard<std::mutex> lock(pool.mutex);
    s.state.store(SlotLife::FREE, std::memory_order_release);
    --pool.nof_open;
  }
  pool.changed.notify_all();
}

// True until the slot is armed: the writers of an open slot ask this under the slot's mutex.
inline bool slot_is_open(const SlotCore& s)
{
  return s.state.load(std::memory_order_acquire) == SlotLife::OPEN;
}

// OPEN -> FINISHING, under the slot's mutex and BEFORE the completion callback is enqueued: slot_pool_complete follows from
// a runtime thread, or slot_fail_armed from the caller if the callback could not be enqueued.
inline void slot_arm(SlotCore& s, slot_done_fn done, void* user)
{
  s.done = done;
  s.user = user;
  s.state.store(SlotLife::FINISHING, std::memory_order_release);
}

// The tail of the stream callback.  The state is DONE before the handler runs, so the handler may poll and read results; the
// empty lock of the pool's mutex orders the state store against a waiter that has tested the state and not yet slept, so
// that no wake-up is lost.  The slot is not touched after the handler returns, only the pool.
template <class Slot>
void slot_pool_complete(SlotPool<Slot>& pool, SlotCore& s, int rc)
{
  s.status.store(rc, std::memory_order_relaxed);
  s.state.store(SlotLife::DONE, std::memory_order_release);
  if (s.done != nullptr) {
    s.done(s.user, rc, s.id);
  }
  {
    std::lock_guard<std::mutex> lock(pool.mutex);
  }
  pool.changed.notify_all();
}

// An armed slot whose callback was never enqueued, after its stream has been synchronised: DONE with NRPHY_ERR_DEVICE, and
// no handler runs.
inline void slot_fail_armed(SlotCore& s)
{
  s.status.store(NRPHY_ERR_DEVICE, std::memory_order_relaxed);
  s.state.store(SlotLife::DONE, std::memory_order_release);
}

// Returns once DONE has been stored for an armed slot: at once unless the slot is FINISHING.  That is all it guarantees: the
// completion callback stores DONE BEFORE it reads the handler and runs it, so that the callback has RETURNED is the caller's
// own knowledge -- the pools synchronise the slot's stream, callbacks included, before they call this and release the slot
// (slot_pool_claim rewrites the handler without the slot's mutex).  The caller holds the slot's mutex.
template <class Slot>
void slot_pool_await_callback(SlotPool<Slot>& pool, const SlotCore& s)
{
  if (s.state.load(std::memory_order_acquire) == SlotLife::FINISHING) {
    std::unique_lock<std::mutex> lock(pool.mutex);
    pool.changed.wait(lock, [&s] { return s.state.load(std::memory_order_acquire) == SlotLife::DONE; });
  }
}

// Never blocks.  DONE: the slot's status; OPEN or FINISHING: NRPHY_ERR_NOT_READY; a free slot, a bad id, no pool:
// NRPHY_ERR_ARGUMENT.
template <class Slot>
int slot_pool_poll(const SlotPool<Slot>* pool, uint32_t slot_id)
{
  if (pool == nullptr || slot_id >= pool->slots.size()) {
    return NRPHY_ERR_ARGUMENT;
  }
  const SlotCore& s = pool->slots[slot_id];
  switch (s.state.load(std::memory_order_acquire)) {
    case SlotLife::DONE:
      return s.status.load(std::memory_order_relaxed);
    case SlotLife::FREE:
      return NRPHY_ERR_ARGUMENT;
    default:
      return NRPHY_ERR_NOT_READY;
  }
}

// Blocks while the slot is FINISHING and returns its status; NRPHY_ERR_ARGUMENT where there is nothing to wait for (an open
// slot, a free one, a bad id, no pool).
template <class Slot>
int slot_pool_wait(SlotPool<Slot>* pool, uint32_t slot_id)
{
  const SlotCore* s = slot_pool_lookup(pool, slot_id);
  if (s == nullptr || s->state.load(std::memory_order_acquire) == SlotLife::OPEN) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::unique_lock<std::mutex> lock(pool->mutex);
  pool->changed.wait(lock, [s] { return s->state.load(std::memory_order_acquire) != SlotLife::FINISHING; });
  return s->state.load(std::memory_order_acquire) == SlotLife::DONE ? s->status.load(std::memory_order_relaxed) : NRPHY_ERR_ARGUMENT;
}

// Blocks until slot_pool_claim would have found a slot (another thread may still take it first).
template <class Slot>
int slot_pool_wait_free(SlotPool<Slot>* pool)
{
  if (pool == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::unique_lock<std::mutex> lock(pool->mutex);
  pool->changed.wait(lock, [pool] { return pool->nof_open < pool->slots.size(); });
  return NRPHY_OK;
}

#pragma GCC visibility pop
