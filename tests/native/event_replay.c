/* sf_missile_events (spacefortress_amd/csrc/sf_events.h, the header the step kernel compiles) against a plain walk of a
 * tick's missile events in slot order, written from SRC/game.cpp:353-402 as oracle/sf_oracle.c:update_missiles restates it.
 * Exhaustive over: fortress alive / dead, fort_vuln_timer {0, 216, 249, 250, 284}, vlner 0..13, every slot-ordered sequence
 * of 0..6 events over {hit, out}, points {0, 0.05f, 0.95f, 7}, both scorings.  Every output and the float bits of
 * reward / raw_points / points must be equal.  gcc -O2 -ffp-contract=off. */
#include <stdio.h>
#include <string.h>

#include "sf_events.h"

enum { VULN_TIME = 250, VULN_THRESHOLD = 10 };

typedef struct {
  int alive, vuln_t, death_t, vlner, incs, resets, destroyed, missed, max_vlner;
  float reward, raw, points;
} game;

static void game_reward(game* g, float amount) { /* :97-102 */
  g->reward += amount;
  g->raw += amount;
  g->points += amount;
  if (g->points < 0) g->points = 0;
}

/* the walk of :355-401 over the events of one env; seq bit k: event k is a hit (else it left the area) */
static void walk(game* g, unsigned seq, int n, float destroy_reward, float miss_penalty) {
  int k;
  for (k = 0; k < n; k++) {
    if ((seq >> k) & 1u) {
      if (g->alive) {
        if (g->vuln_t >= VULN_TIME) {
          g->vlner += 1;
          g->incs += 1;
          if (g->vlner > g->max_vlner) g->max_vlner = g->vlner;
        } else {
          if (g->vlner >= VULN_THRESHOLD + 1) {
            g->alive = 0;
            g->death_t = 0;
            game_reward(g, destroy_reward);
            g->destroyed += 1;
          } else {
            g->resets += 1;
          }
          g->vlner = 0;
        }
        g->vuln_t = 0;
      }
    } else {
      game_reward(g, -miss_penalty);
      g->missed += 1;
    }
  }
}

static unsigned bits(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return u;
}

int main(void) {
  static const int vts[] = {0, 216, 249, 250, 284};
  static const float pts[] = {0.0f, 0.05f, 0.95f, 7.0f};
  long cases = 0, bad = 0;
  int shaped, alive, vi, vlner, n, pi;
  unsigned seq;
  for (shaped = 0; shaped < 2; shaped++) {
    const float destroy_reward = shaped ? 1.0f : 100.0f; /* sf_layout.h: sfc::Score<SHAPED> */
    for (alive = 0; alive < 2; alive++)
      for (vi = 0; vi < 5; vi++)
        for (vlner = 0; vlner <= 13; vlner++)
          for (n = 0; n <= 6; n++)
            for (seq = 0; seq < (1u << n); seq++)
              for (pi = 0; pi < 4; pi++) {
                game a, b;
                SfMissileEvents e;
                int k, n_hit = 0, same;
                memset(&a, 0, sizeof a);
                a.alive = alive;
                a.vuln_t = vts[vi];
                a.death_t = 777;
                a.vlner = vlner;
                a.points = pts[pi];
                a.raw = pts[pi] - 1.0f;
                a.reward = shaped ? -0.05f : -2.0f; /* a tick's earlier amount: the fire penalty */
                b = a;
                walk(&a, seq, n, destroy_reward, 0.0f);
                for (k = 0; k < n; k++) n_hit += (seq >> k) & 1u;
                e = sf_missile_events(n_hit, n - n_hit, b.alive, b.vuln_t, b.vlner, VULN_TIME, VULN_THRESHOLD, destroy_reward);
                /* what the kernel does with the outputs */
                b.vlner = e.vlner;
                b.alive = e.fort_alive;
                b.vuln_t = e.fort_vuln_t;
                b.death_t = e.fort_death_reset ? 0 : b.death_t;
                b.incs += e.incs;
                b.max_vlner = e.max_vlner > b.max_vlner ? e.max_vlner : b.max_vlner;
                b.destroyed += e.destroyed;
                b.resets += e.resets;
                b.missed += e.missed;
                game_reward(&b, e.amount);
                same = a.alive == b.alive && a.vuln_t == b.vuln_t && a.death_t == b.death_t && a.vlner == b.vlner &&
                       a.incs == b.incs && a.resets == b.resets && a.destroyed == b.destroyed && a.missed == b.missed &&
                       a.max_vlner == b.max_vlner && bits(a.reward) == bits(b.reward) && bits(a.raw) == bits(b.raw) &&
                       bits(a.points) == bits(b.points);
                cases++;
                if (!same && bad++ < 10)
                  printf("differs: shaped %d alive %d vuln_t %d vlner %d n %d seq 0x%x points %g\n", shaped, alive, vts[vi],
                         vlner, n, seq, (double)pts[pi]);
              }
  }
  printf("mismatches=%ld of %ld\n", bad, cases);
  return bad != 0;
}
