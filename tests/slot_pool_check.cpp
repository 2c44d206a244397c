// Stand-alone check of csrc/slot_pool_host.h (no GPU, no HIP): the life cycle that the downlink and the uplink slot pools share,
// exactly as dl_slot_async.cpp and ul_slot_async.cpp use it.  Built and run by tests/test_slot_pool_host.py, once plainly, once
// under the address and undefined-behaviour sanitizers and once under the thread sanitizer.  Plain std::threads stand in for the
// threads of the HIP runtime that run the completion callbacks; a lost wake-up shows as a run that never ends.
#include "slot_pool_host.h"

#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#define CHECK(cond)                                                                                                    \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                                    \
      std::exit(1);                                                                                                    \
    }                                                                                                                  \
    checks.fetch_add(1, std::memory_order_relaxed);                                                                    \
  } while (0)

static std::atomic<unsigned> checks{0};

namespace { // (the header's types are hidden: what derives from them stays inside this file)

struct Slot : SlotCore {
  std::atomic<uint32_t> owner{0};       // 0: nobody, else the thread that claimed it
  std::atomic<bool>     returned{true}; // the completion callback has returned (what hipStreamSynchronize waits for in a pool)
  int                   rc_given   = 0; // what the slot is completed with
  bool                  wait_first = false; // whoever closes it calls wait before
};

struct Pool : SlotPool<Slot> {
  explicit Pool(uint32_t depth)
  {
    slots       = std::vector<Slot>(depth);
    uint32_t id = 0;
    for (Slot& s : slots) {
      s.id = id++;
    }
  }
  uint32_t open_now()
  {
    std::lock_guard<std::mutex> lock(mutex);
    return nof_open;
  }
};

// What a handler is given as `user`: it checks its arguments against what the slot was armed and completed with.
struct Handled {
  Pool*                 pool = nullptr;
  std::atomic<uint32_t> calls{0}, last_id{0xFFFFFFFFu};
};

void on_done(void* user, int status, uint32_t slot_id)
{
  Handled* h = static_cast<Handled*>(user);
  CHECK(slot_id < h->pool->slots.size());
  const Slot& s = h->pool->slots[slot_id];
  CHECK(s.user == user && status == s.rc_given);
  CHECK(slot_pool_poll(h->pool, slot_id) == status); // the state was stored before the handler runs
  h->last_id.store(slot_id);
  h->calls.fetch_add(1);
}

// ---- every transition, one thread --------------------------------------------------------------------------------------------
void transitions(uint32_t depth)
{
  Pool    pool(depth);
  Handled handled;
  handled.pool = &pool;
  CHECK(pool.open_now() == 0);
  CHECK(slot_pool_lookup(&pool, 0) == nullptr && slot_pool_lookup(&pool, depth) == nullptr); // free, bad id
  CHECK(slot_pool_lookup(static_cast<Pool*>(nullptr), 0) == nullptr);
  CHECK(slot_pool_poll(&pool, 0) == NRPHY_ERR_ARGUMENT && slot_pool_poll(&pool, depth) == NRPHY_ERR_ARGUMENT);
  CHECK(slot_pool_poll(&pool, 0xFFFFFFFFu) == NRPHY_ERR_ARGUMENT && slot_pool_poll(static_cast<Pool*>(nullptr), 0) == NRPHY_ERR_ARGUMENT);
  CHECK(slot_pool_wait(&pool, 0) == NRPHY_ERR_ARGUMENT && slot_pool_wait(&pool, depth) == NRPHY_ERR_ARGUMENT);
  CHECK(slot_pool_wait(static_cast<Pool*>(nullptr), 0) == NRPHY_ERR_ARGUMENT);
  CHECK(slot_pool_wait_free(static_cast<Pool*>(nullptr)) == NRPHY_ERR_ARGUMENT && slot_pool_wait_free(&pool) == NRPHY_OK);

  // claim `depth` times: distinct ids, in order; once more: none
  std::vector<bool> seen(depth, false);
  for (uint32_t k = 0; k != depth; ++k) {
    Slot* s = slot_pool_claim(pool);
    CHECK(s != nullptr && s->id < depth && !seen[s->id] && s == &pool.slots[s->id]);
    seen[s->id] = true;
    CHECK(pool.open_now() == k + 1);
    CHECK(slot_pool_lookup(&pool, s->id) == s && slot_is_open(*s));
    CHECK(slot_pool_poll(&pool, s->id) == NRPHY_ERR_NOT_READY); // OPEN
    CHECK(slot_pool_wait(&pool, s->id) == NRPHY_ERR_ARGUMENT);  // nothing to wait for
  }
  CHECK(slot_pool_claim(pool) == nullptr && pool.open_now() == depth);
  CHECK(slot_pool_lookup(&pool, depth) == nullptr);

  // every slot through arm and complete, with both statuses, with and without a handler; then fail_armed; then release
  uint32_t want_calls = 0;
  for (uint32_t id = 0; id != depth; ++id) {
    Slot& s = pool.slots[id];
    for (uint32_t round = 0; round != 5; ++round) {
      const int  rc      = round % 2 == 0 ? NRPHY_OK : NRPHY_ERR_DEVICE;
      const bool handler = round < 2;
      if (round != 0) { // (round 0 uses the claim above)
        CHECK(slot_pool_claim(pool) == &s);
        CHECK(s.done == nullptr && s.user == nullptr); // no stale handler ...
        CHECK(slot_pool_poll(&pool, id) == NRPHY_ERR_NOT_READY && s.status.load() == NRPHY_OK); // ... and no stale status
      }
      CHECK(pool.open_now() == depth);
      s.rc_given = rc;
      slot_arm(s, handler ? on_done : nullptr, handler ? &handled : nullptr);
      CHECK(!slot_is_open(s) && slot_pool_lookup(&pool, id) == &s);
      CHECK(slot_pool_poll(&pool, id) == NRPHY_ERR_NOT_READY); // FINISHING
      if (round == 4) {
        slot_fail_armed(s); // the callback could not be enqueued: no handler runs
        CHECK(slot_pool_poll(&pool, id) == NRPHY_ERR_DEVICE && slot_pool_wait(&pool, id) == NRPHY_ERR_DEVICE);
      } else {
        slot_pool_complete(pool, s, rc);
        want_calls += handler;
        CHECK(!handler || handled.last_id.exchange(0xFFFFFFFFu) == id);
        CHECK(slot_pool_poll(&pool, id) == rc && slot_pool_wait(&pool, id) == rc); // DONE
      }
      CHECK(handled.calls.load() == want_calls);
      CHECK(!slot_is_open(s) && pool.open_now() == depth);
      slot_pool_await_callback(pool, s); // DONE: returns at once
      slot_pool_release(pool, s);
      CHECK(pool.open_now() == depth - 1);
      CHECK(slot_pool_lookup(&pool, id) == nullptr && slot_pool_poll(&pool, id) == NRPHY_ERR_ARGUMENT); // FREE
      CHECK(slot_pool_wait(&pool, id) == NRPHY_ERR_ARGUMENT && slot_pool_wait_free(&pool) == NRPHY_OK);
    }
    // an open slot given back without having been armed (uplink open's failure path); the next claim takes the lowest free id
    CHECK(slot_pool_claim(pool) == &s && pool.open_now() == depth);
    slot_pool_release(pool, s);
    CHECK(pool.open_now() == depth - 1);
    CHECK(slot_pool_claim(pool) == &s && slot_is_open(s) && pool.open_now() == depth);
  }
  for (Slot& s : pool.slots) {
    slot_pool_release(pool, s);
  }
  CHECK(pool.open_now() == 0 && handled.calls.load() == 2 * depth);
}

// ---- several threads ---------------------------------------------------------------------------------------------------------
struct Rng {
  uint32_t x;
  uint32_t next()
  {
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    return x;
  }
};

// Slots handed from thread to thread; nullptr ends the reader.
struct Queue {
  std::mutex              mutex;
  std::condition_variable filled;
  std::deque<Slot*>       items;
  void push(Slot* s)
  {
    {
      std::lock_guard<std::mutex> lock(mutex);
      items.push_back(s);
    }
    filled.notify_one();
  }
  Slot* pop()
  {
    std::unique_lock<std::mutex> lock(mutex);
    filled.wait(lock, [this] { return !items.empty(); });
    Slot* s = items.front();
    items.pop_front();
    return s;
  }
};

struct Run {
  Pool                  pool;
  Handled               handled;
  Queue                 runtime[2], closer;
  std::atomic<uint32_t> armed_with_handler{0}, closed{0};
  explicit Run(uint32_t depth) : pool(depth) { handled.pool = &pool; }
};

// What nrphy_*_slot_close does, with the calls of the header in its order, behind nrphy_*_slot_wait or, as a caller may, without.
void close_slot(Run& run, Slot* s)
{
  if (s->wait_first) {
    CHECK(slot_pool_wait(&run.pool, s->id) == s->rc_given);
  }
  {
    std::lock_guard<std::mutex> lock(s->mutex);
    slot_pool_await_callback(run.pool, *s); // blocks where nobody has waited yet
    CHECK(slot_pool_poll(&run.pool, s->id) == s->rc_given);
    while (!s->returned.load(std::memory_order_acquire)) { // (the stream synchronise of a pool: the callback has returned)
      std::this_thread::yield();
    }
  }
  CHECK(s->owner.exchange(0) != 0);
  slot_pool_release(run.pool, *s);
  run.closed.fetch_add(1);
}

void submitter(Run& run, uint32_t me, uint32_t nof_slots, uint32_t seed)
{
  Rng            rng{seed};
  const uint32_t depth = (uint32_t)run.pool.slots.size();
  for (uint32_t k = 0; k != nof_slots;) {
    Slot* s = slot_pool_claim(run.pool);
    if (s == nullptr) {
      (void)slot_pool_wait_free(&run.pool); // (not counted: how often a submitter gets here differs from run to run)
      continue;
    }
    ++k;
    CHECK(s->owner.exchange(me) == 0); // nobody else holds it
    const uint32_t open_now = run.pool.open_now();
    CHECK(open_now >= 1 && open_now <= depth);
    const uint32_t r = rng.next();
    {
      std::lock_guard<std::mutex> lock(s->mutex);
      CHECK(slot_is_open(*s) && s->done == nullptr && s->status.load() == NRPHY_OK);
      s->rc_given   = (r & 1) != 0 ? NRPHY_OK : NRPHY_ERR_DEVICE;
      s->wait_first = (r & 16) != 0;
      s->returned.store(false, std::memory_order_relaxed);
      const bool handler = (r & 2) != 0;
      run.armed_with_handler.fetch_add(handler);
      slot_arm(*s, handler ? on_done : nullptr, handler ? &run.handled : nullptr);
    }
    run.runtime[(r >> 2) & 1].push(s);
    if ((r & 8) != 0) {
      run.closer.push(s);
    } else {
      close_slot(run, s);
    }
  }
}

// A thread of the runtime: the completion callback of each slot it is handed, some time later.
void runtime_thread(Run& run, Queue& queue, uint32_t seed)
{
  Rng rng{seed};
  while (Slot* s = queue.pop()) {
    for (uint32_t spins = rng.next() % 8; spins != 0; --spins) {
      std::this_thread::yield();
    }
    slot_pool_complete(run.pool, *s, s->rc_given);
    s->returned.store(true, std::memory_order_release);
  }
}

void closer_thread(Run& run)
{
  while (Slot* s = run.closer.pop()) {
    close_slot(run, s);
  }
}

void several_threads(uint32_t depth, uint32_t seed)
{
  const uint32_t nof_submitters = 4, nof_slots = 300;
  Run            run(depth);
  std::thread    r0(runtime_thread, std::ref(run), std::ref(run.runtime[0]), seed + 100);
  std::thread    r1(runtime_thread, std::ref(run), std::ref(run.runtime[1]), seed + 200);
  std::thread    closer(closer_thread, std::ref(run));
  std::vector<std::thread> submitters;
  for (uint32_t i = 0; i != nof_submitters; ++i) {
    submitters.emplace_back(submitter, std::ref(run), i + 1, nof_slots, seed + i + 1);
  }
  for (std::thread& t : submitters) {
    t.join();
  }
  run.closer.push(nullptr);
  closer.join();
  run.runtime[0].push(nullptr);
  run.runtime[1].push(nullptr);
  r0.join();
  r1.join();
  CHECK(run.closed.load() == nof_submitters * nof_slots);
  CHECK(run.pool.open_now() == 0);
  CHECK(run.handled.calls.load() == run.armed_with_handler.load());
  for (uint32_t id = 0; id != depth; ++id) {
    CHECK(slot_pool_lookup(&run.pool, id) == nullptr && run.pool.slots[id].owner.load() == 0);
  }
  Slot* s = slot_pool_claim(run.pool);
  CHECK(s != nullptr && s->id == 0 && s->done == nullptr && s->status.load() == NRPHY_OK);
}

} // namespace

int main()
{
  const uint32_t depths[] = {1, 2, 64};
  for (uint32_t depth : depths) {
    transitions(depth);
  }
  several_threads(1, 0x1234567u);
  several_threads(2, 0x89ABCDEu);
  several_threads(4, 0x2468ACEu);
  std::printf("ok: %u checks\n", checks.load());
  return 0;
}
