// What a tick's missile events do to the fortress and the score (SRC/game.cpp:353-402), in closed form.
//
// The reference walks the missile slots in order; every missile that reaches the fortress or leaves the area is an event.
// The walk is a pure function of how MANY hits and misses there are, the fortress state and vlner:
//   - a miss only counts (its penalty is 0, and x + (-0.0f) == x bit for bit), so where it stands among the hits is moot;
//   - the first hit on a live fortress sets fort_vuln_timer to 0, so every later hit of the same tick falls inside the
//     vulnerability window: the second destroys or resets, and every further hit on a fortress still alive resets a vlner
//     that is already 0;
//   - a hit on a dead fortress does nothing, and a fortress destroyed in this walk stays dead for the rest of it.
// So at most one non-zero amount (the destruction) is scored, and nothing is scored behind it.
//
// Plain C, no HIP types: the step kernel includes this, and so does tests/native/event_replay.c with gcc, which holds it to a
// slot-order loop over every case.  SF_EVENTS_FN is the function qualifier.
#pragma once

#ifndef SF_EVENTS_FN
#define SF_EVENTS_FN static inline
#endif

typedef struct SfMissileEvents {
  int vlner;             // the new vlner
  int fort_alive;        // the fortress after the walk
  int fort_vuln_t;       // the new fort_vuln_timer (0 after any hit on a live fortress)
  int fort_death_reset;  // fort_death_timer = 0 (the fortress was destroyed)
  int incs, resets, destroyed, missed;  // this walk's share of the statistics
  int max_vlner;         // candidate for the running maximum of vlner (0: none)
  float amount;          // the one amount to score: destroy_reward or 0.0f
} SfMissileEvents;

// n_hit / n_out: live missiles that reached the fortress / left the game area this tick.  Selects only.
SF_EVENTS_FN SfMissileEvents sf_missile_events(int n_hit, int n_out, int fort_alive, int fort_vuln_t, int vlner, int vuln_time,
                                               int vuln_threshold, float destroy_reward) {
  SfMissileEvents e;
  // first hit on a live fortress (:358-386)
  const int h1 = (n_hit >= 1) & (fort_alive != 0);
  const int inc = h1 & (fort_vuln_t >= vuln_time);               // :359-363
  const int low1 = h1 & !inc;                                    // inside the window (:364-384)
  const int destroy1 = low1 & (vlner >= vuln_threshold + 1);
  const int v1 = inc ? vlner + 1 : (low1 ? 0 : vlner);
  // second hit: the timer is 0 now, so it is inside the window
  const int h2 = (n_hit >= 2) & h1 & !destroy1;
  const int destroy2 = h2 & (v1 >= vuln_threshold + 1);
  // hits 3..n on a fortress still alive: resets of vlner == 0
  const int h3 = h2 & !destroy2;
  const int more = (h3 && n_hit > 2) ? n_hit - 2 : 0;
  const int destroyed = destroy1 | destroy2;
  e.vlner = h2 ? 0 : v1;
  e.fort_alive = (fort_alive != 0) & !destroyed;
  e.fort_vuln_t = h1 ? 0 : fort_vuln_t;
  e.fort_death_reset = destroyed;
  e.incs = inc;
  e.resets = (low1 & !destroy1) + (h2 & !destroy2) + more;
  e.destroyed = destroyed;
  e.missed = n_out;
  e.max_vlner = inc ? v1 : 0;
  e.amount = destroyed ? destroy_reward : 0.0f;
  return e;
}
