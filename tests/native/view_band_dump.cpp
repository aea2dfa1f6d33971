// Prints what sf_view_resolve (sf_view_host.cpp) makes of views read from the command line -- width height vp_x vp_y vp_w vp_h
// line_width grayscale, eight numbers per view -- one line per view: "w h planes band_h circle_k", or "error <code>".  For
// tests/test_view_edges_model.py to hold the Python restatement of the band rule to.  Host only: sf_view_host.cpp makes no HIP
// calls (its headers are HIP's for their types); the three functions it takes from other translation units are stood in for
// here -- resolving a view without an atlas calls none of them but sf_set_error.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include "sf_internal.h"
#include "sf_view.h"

void sf_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}
int sf_glyphs_pack(const sf_score_glyphs*, const uint8_t*, const int*, SfGlyphAtlas*) { return SF_ERR_ARG; }
extern "C" int sf_image_background_geom(int, int, double, double, double, double, double, uint8_t*) { return SF_ERR_ARG; }

int main(int argc, char** argv) {
  for (int i = 1; i + 8 <= argc; i += 8) {
    sf_view v = {};
    v.width = atoi(argv[i]);
    v.height = atoi(argv[i + 1]);
    v.vp_x = atof(argv[i + 2]);
    v.vp_y = atof(argv[i + 3]);
    v.vp_w = atof(argv[i + 4]);
    v.vp_h = atof(argv[i + 5]);
    v.line_width = atof(argv[i + 6]);
    v.grayscale = atoi(argv[i + 7]);
    v.format = SF_VIEW_BGRX;
    SfViewRes r;
    const int rc = sf_view_resolve(&v, 710, 626, &r);
    if (rc != SF_OK) printf("error %d\n", rc);
    else printf("%d %d %d %d %d\n", r.w, r.h, r.planes, r.band_h, r.circle_k);
  }
  return 0;
}
