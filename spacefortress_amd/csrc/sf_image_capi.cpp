// sf_image_capi.cpp -- the C ABI of include/sfmi.h, everything that draws: the image observation's tables, pictures, glyph atlas
// and geometry, the frames, the view cache.  Host code only; the kernels are in sf_render.hip, sf_render_generic.hip,
// sf_render_view.hip and (the draw records from the state) sf_state_ops.hip.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sf_batch.h"
#include "sf_drawrec.h"
#include "sf_raster.h"

namespace {

// b->d_xcache behind the envs' explosion cache (n_envs * SF_XC_BYTES), as byte offsets: the 36 fortress pictures, the destroyed
// fortress's explosion (in the layout of an env's cache entry), the score / bar pictures; and the whole allocation's size
struct PictureTail { size_t fort, destroyed, hud, total; };
PictureTail picture_tail(const sf_batch* b) {
  const size_t fort = (size_t)b->n_envs * SF_XC_BYTES, destroyed = fort + 36 * SF_FP_BYTES, hud = destroyed + SF_XC_BYTES;
  return {fort, destroyed, hud, hud + SF_HUD_BYTES};
}
// ... and the pictures drawn into the (zeroed) tail, by the frame kernel's own code
int draw_pictures(sf_batch* b, hipStream_t stream) {
  const PictureTail t = picture_tail(b);
  HIP_TRY(sf_launch_hud_pictures(b->d_bg.get(), b->d_bg84.get(), b->d_tabs.get(), b->d_xcache.get() + t.hud, b->d_glyphs.get(), stream));
  HIP_TRY(sf_launch_fort_patches(b->d_bg.get(), b->d_bg84.get(), b->d_tabs.get(), b->d_xcache.get() + t.fort, b->d_arcs.get(),
                                 b->d_falpha.get(), stream));
  return SF_OK;
}

// What the default geometry's frame kernel keeps of the score text, (re)made from b->h_glyphs: the four static backgrounds
// (variant bit 0 = the score 0000000 baked in) with their 84x84 images and -- where they exist already -- the explosion
// cache, the score / bar pictures and the backgrounds with the fortress in them.  Synchronous.
int bake_default_glyphs(sf_batch* b) {
  std::vector<uint8_t> bg(4 * SF_BG_STRIDE, 0), bg84(4 * SF_OUT * SF_OUT);
  for (int v = 0; v < 4; v++) {  // static background variants: sf_raster.h
    int rc = sf_image_static_glyphs(v, &b->h_glyphs, bg.data() + v * SF_BG_STRIDE);
    if (rc == SF_OK) rc = sf_resize_area_u8(bg.data() + v * SF_BG_STRIDE, SF_IMG_W, SF_IMG_H, bg84.data() + v * SF_OUT * SF_OUT, SF_OUT, SF_OUT);
    if (rc != SF_OK) return rc;
  }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(b->d_bg84.get(), bg84.data(), bg84.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->d_bg.get(), bg.data(), bg.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->d_glyphs.get(), &b->h_glyphs, sizeof(SfGlyphAtlas), hipMemcpyHostToDevice));
  b->baked_glyphs = b->h_glyphs;
  if (b->render_ready && b->d_xcache) {
    HIP_TRY(hipMemset(b->d_xcache.get(), 0, picture_tail(b).total));
    SF_TRY(draw_pictures(b, nullptr));
    HIP_TRY(hipDeviceSynchronize());
  }
  b->draw_current = false;
  return SF_OK;
}

// `count` T on the device, holding what `host` holds
template <typename T>
int upload(DevBuf<T>& d, const T* host, size_t count) {
  HIP_TRY(d.alloc(count));
  HIP_TRY(hipMemcpy(d.get(), host, count * sizeof(T), hipMemcpyHostToDevice));
  return SF_OK;
}

}  // namespace

// The envs' draw records from the state as it is (sf_drawrec_kernel), into b->d_draw, which exists.  Current afterwards for an
// image batch, whose step launches keep them so; a batch that steps with a symbolic observation rebuilds before every frame.
int sfb_rebuild_draw_records(sf_batch* b, hipStream_t stream) {
  SfKernelArgs da = b->args;
  da.draw = b->d_draw.get();
  da.draw_pics = b->d_xcache ? 1 : 0;
  HIP_TRY(sf_launch_drawrec(da, stream));
  b->draw_current = b->args.draw != nullptr;
  return SF_OK;
}

// What a batch needs to draw frames, made once: the per-env explosion cache followed by the 36 fortress pictures, the
// destroyed fortress's explosion (in the layout of an env's cache entry) and the score / bar pictures -- all drawn here, on
// `stream`, by the frame kernel's own code; the 36 x 4 backgrounds with the fortress in them; the envs' draw records.
// Image batches call this from sf_create and wait for it (every later launch, on whatever stream, finds the pictures
// finished: a first frame inside a HIP-graph capture allocates nothing); other batches with their first frame.
// SFMI_NO_EXPLOSION_CACHE (diagnostics, tools/render_soak.py): no caches, no pictures -- every frame drawn in place.
int sfb_ensure_render_resources(sf_batch* b, hipStream_t stream) {
  if (b->render_ready) return SF_OK;
  if (!b->d_draw) {
    const size_t bytes = (size_t)b->args.lanes * SF_DR_BYTES;
    HIP_TRY(b->d_draw.alloc(bytes));
    HIP_TRY(hipMemsetAsync(b->d_draw.get(), 0, bytes, stream));
  }
  if (!b->d_xcache && !getenv("SFMI_NO_EXPLOSION_CACHE")) {
    const size_t total = picture_tail(b).total;
    HIP_TRY(b->d_xcache.alloc(total));
    HIP_TRY(hipMemsetAsync(b->d_xcache.get(), 0, total, stream));
    SF_TRY(draw_pictures(b, stream));
  }
  HIP_TRY(hipStreamSynchronize(stream));
  b->render_ready = true;
  b->draw_current = false;
  return SF_OK;
}

// The image observation tables of a new batch (sf_image.cpp): 101 KB, built for every batch so that sf_render works whatever
// obs_type the batch steps with (the reference's render(), ENV:190-193)
int sfb_create_image_tables(sf_batch* b) {
  static_assert(SF_IMG_W == SF_IMAGE_W && SF_IMG_H == SF_IMAGE_H && SF_OUT == SF_IMAGE_OUT, "sfmi.h vs sf_raster.h");
  static_assert(SF_IMG_W == (int)sfc::pb_width && SF_IMG_H == (int)sfc::pb_height, "ENV:57-58");
  uint32_t tabs[SF_TAB_WORDS];  // device layout of the INTER_AREA tables: sf_raster.h
  SF_TRY(sf_area_tabs_default(tabs));
  // (room for the backgrounds with the fortress in them, filled by the first frame: sf_launch_fort_patches)
  HIP_TRY(b->d_bg84.alloc((size_t)SF_BG_COUNT * SF_OUT * SF_OUT / sizeof(uint32_t)));
  HIP_TRY(hipMemset(b->d_bg84.get(), 0, (size_t)SF_BG_COUNT * SF_OUT * SF_OUT));
  HIP_TRY(b->d_bg.alloc((size_t)SF_BG_COUNT * SF_BG_STRIDE / sizeof(uint32_t)));
  HIP_TRY(hipMemset(b->d_bg.get(), 0, (size_t)SF_BG_COUNT * SF_BG_STRIDE));
  static_assert(SF_OUT * SF_OUT % sizeof(uint32_t) == 0 && SF_BG_STRIDE % sizeof(uint32_t) == 0, "backgrounds in whole words");
  std::vector<double> arcs(86 * 8);
  SF_TRY(sf_arc_table(arcs.data()));
  const uint8_t* fa = sf_fort_alpha_table();
  if (!fa) return SF_ERR_ARG;
  SF_TRY(upload(b->d_arcs, arcs.data(), arcs.size()));
  SF_TRY(upload(b->d_falpha, fa, (size_t)360 * 256));
  SF_TRY(upload(b->d_tabs, tabs, (size_t)SF_TAB_WORDS));
  // the score text: the built-in glyph atlas (sf_glyphs.h) and the four static backgrounds made with it
  HIP_TRY(b->d_glyphs.alloc(1));
  sf_glyphs_default(&b->h_glyphs);
  return bake_default_glyphs(b);
}

extern "C" int sf_set_render_order_hint(sf_batch* b, const uint64_t* words_host, int n_words) {
  if (!b || !words_host || !b->args.hint || n_words != (b->n_envs + 63) / 64) {
    sf_set_error("sf_set_render_order_hint: needs an image batch and ceil(n_envs / 64) words");
    return SF_ERR_ARG;
  }
  DeviceGuard guard(b->device);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(b->args.hint, words_host, (size_t)n_words * sizeof(uint64_t), hipMemcpyHostToDevice));
  return SF_OK;
}

extern "C" int sf_image_size(const sf_batch* b, int32_t* width, int32_t* height) {
  if (!b || !width || !height) return SF_ERR_ARG;
  *width = b->g_w ? b->g_w : SF_IMG_W;
  *height = b->g_w ? b->g_h : SF_IMG_H;
  return SF_OK;
}

extern "C" int sf_image_geometry_is_default(const sf_batch* b) { return b && b->g_w == 0 ? 1 : 0; }

extern "C" int sf_set_image_geometry(sf_batch* b, double scale, double vp_x, double vp_y, double vp_w, double vp_h, double line_width) {
  if (!b) {
    sf_set_error("sf_set_image_geometry: null batch");
    return SF_ERR_ARG;
  }
  if (!(scale > 0) || !(vp_w > 0) || !(vp_h > 0) || !(line_width > 0) || !(vp_w * scale < 1e6) || !(vp_h * scale < 1e6)) {
    sf_set_error("sf_set_image_geometry: scale, viewport size and line width must be positive");
    return SF_ERR_ARG;
  }
  const int w = (int)(vp_w * scale), h = (int)(vp_h * scale);  // ENV:57-58
  DeviceGuard guard(b->device);
  HIP_TRY(hipDeviceSynchronize());
  if (vp_x == SF_VP_X && vp_y == SF_VP_Y && vp_w == 450.0 && vp_h == 460.0 && w == SF_IMG_W && h == SF_IMG_H && line_width == SF_LINE_W) {
    b->g_w = b->g_h = 0;  // the default geometry: the fast frame kernel, the built-in glyph atlas
    sf_glyphs_default(&b->h_glyphs);
    if (memcmp(&b->h_glyphs, &b->baked_glyphs, sizeof(SfGlyphAtlas)) != 0) return bake_default_glyphs(b);
    HIP_TRY(hipMemcpy(b->d_glyphs.get(), &b->h_glyphs, sizeof(SfGlyphAtlas), hipMemcpyHostToDevice));
    return SF_OK;
  }
  if (w < SF_OUT || h < SF_OUT || w >= 3 * SF_OUT || h >= 3 * SF_OUT || (long)w * h > 49152) {
    sf_set_error("sf_set_image_geometry: a %d x %d surface (scale %g, viewport %g x %g): width and height must lie in [%d, %d] "
                 "with width * height <= 49152 (the 84x84 INTER_AREA image of the trainer is a shrink below threefold)",
                 w, h, scale, vp_w, vp_h, SF_OUT, 3 * SF_OUT - 1);
    return SF_ERR_ARG;
  }
  // cairo cuts an arc into Bezier segments by the tolerance over its DEVICE radius (cairo-arc.c: _arc_segments_needed): the
  // explosion's radius-7 circle is one segment per half up to 5.4 device pixels, and that is the form the renderer draws
  if (!((double)w / vp_w <= 0.75) || !((double)h / vp_h <= 0.75)) {
    sf_set_error("sf_set_image_geometry: %d x %d pixels for a %g x %g viewport: more than 0.75 pixels per unit is a close-up "
                 "this renderer does not draw (the explosion's circle takes more Bezier segments there)", w, h, vp_w, vp_h);
    return SF_ERR_ARG;
  }
  std::vector<uint8_t> bg(((size_t)w * h + 15) & ~(size_t)15, 0);  // (whole 16-byte pieces: the kernel copies it that way)
  SF_TRY(sf_image_background_geom(w, h, vp_x, vp_y, vp_w, vp_h, line_width, bg.data()));
  uint32_t tabs[16 * SF_OUT];
  SF_TRY(sf_area_tabs_geom(w, h, tabs));
  DevBuf<uint8_t> nbg;  // the batch keeps its geometry unless both new tables are on the device
  DevBuf<uint32_t> ntabs;
  HIP_TRY(nbg.alloc(bg.size()));
  if (ntabs.alloc(16 * SF_OUT) != hipSuccess || hipMemcpy(nbg.get(), bg.data(), bg.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(ntabs.get(), tabs, sizeof(tabs), hipMemcpyHostToDevice) != hipSuccess) {
    sf_set_error("sf_set_image_geometry: device allocation / copy failed");
    return SF_ERR_HIP;
  }
  b->d_gbg = std::move(nbg);
  b->d_gtabs = std::move(ntabs);
  b->g_w = w;
  b->g_h = h;
  b->g_sx = (double)w / vp_w;
  b->g_sy = (double)h / vp_h;
  b->g_vx = vp_x;
  b->g_vy = vp_y;
  b->g_lw = line_width;
  // no glyph atlas is known for this geometry: the seven-segment fallback until sf_set_score_glyphs gives one
  memset(&b->h_glyphs, 0, sizeof(SfGlyphAtlas));
  HIP_TRY(hipMemcpy(b->d_glyphs.get(), &b->h_glyphs, sizeof(SfGlyphAtlas), hipMemcpyHostToDevice));
  return SF_OK;
}

extern "C" int sf_set_score_glyphs(sf_batch* b, const sf_score_glyphs* layout, const uint8_t* alpha) {
  if (!b) {
    sf_set_error("sf_set_score_glyphs: null batch");
    return SF_ERR_ARG;
  }
  SfGlyphAtlas G;
  const int box[4] = {SF_TXT_BOX_X0, SF_TXT_BOX_Y0, SF_TXT_BOX_X1, SF_TXT_BOX_Y1};
  const int rc = sf_glyphs_pack(layout, alpha, b->g_w ? nullptr : box, &G);
  if (rc != SF_OK) return rc;
  DeviceGuard guard(b->device);
  HIP_TRY(hipDeviceSynchronize());
  b->h_glyphs = G;
  if (!b->g_w) return bake_default_glyphs(b);
  HIP_TRY(hipMemcpy(b->d_glyphs.get(), &b->h_glyphs, sizeof(SfGlyphAtlas), hipMemcpyHostToDevice));
  return SF_OK;
}

extern "C" int sf_get_score_glyphs(const sf_batch* b, int32_t* has_atlas, sf_score_glyphs* layout, uint8_t* alpha, size_t alpha_bytes) {
  if (!b || !has_atlas) {
    sf_set_error("sf_get_score_glyphs: null argument");
    return SF_ERR_ARG;
  }
  const SfGlyphAtlas& G = b->h_glyphs;
  *has_atlas = G.gw ? 1 : 0;
  if (!G.gw) return SF_OK;
  const size_t need = (size_t)SF_GLYPH_CHARS * G.gw * G.gh;
  if (!layout || !alpha || alpha_bytes < need) {
    sf_set_error("sf_get_score_glyphs: need layout and %zu bytes for alpha", need);
    return SF_ERR_ARG;
  }
  layout->gw = G.gw;
  layout->gh = G.gh;
  layout->advance = G.advance;
  layout->y0 = G.y0;
  for (int i = 0; i < SF_GLYPH_CHARS * 10; i++) layout->x0[i / 10][i % 10] = G.x0[i];
  memcpy(alpha, G.alpha, need);
  return SF_OK;
}

int sfb_render(sf_batch* b, int mode, uint8_t* frames_dev, size_t env_stride, hipStream_t stream, const uint8_t* stack_done,
               int stack_slot, int stack_n, const uint8_t* stack_prev) {
  const size_t frame = mode == SF_OBS_IMAGE ? (size_t)SF_OUT * SF_OUT
                                            : (b->g_w ? (size_t)b->g_w * b->g_h : (size_t)SF_IMG_W * SF_IMG_H);
  if (b->g_w) {  // another geometry than the default: the general renderer (sf_render_generic.hip), from the state
    if (env_stride == 0) env_stride = frame;
    if (env_stride < frame) {
      sf_set_error("image frames: env_stride %zu below the frame size %zu", env_stride, frame);
      return SF_ERR_ARG;
    }
    if (stack_prev) {
      sf_set_error("sf_render_shift is built for the default image geometry; use sf_render_stack with this one");
      return SF_ERR_ARG;
    }
    // (the general renderer writes an 84x84 frame in 32-bit words; the surface itself goes out with byte heads and tails)
    if (mode == SF_OBS_IMAGE && ((((uintptr_t)frames_dev) | env_stride) & 3) != 0) {
      sf_set_error("image frames of a non-default geometry must be 4-byte aligned and env_stride a multiple of 4");
      return SF_ERR_ARG;
    }
    // (sf_stack_clear_kernel zeroes a finished env's stack in 16-byte pieces, from the stack's own start)
    if (stack_done && (((uintptr_t)frames_dev - (size_t)stack_slot * frame) & 15) != 0) {
      sf_set_error("sf_render_stack: a stack with done flags must be 16-byte aligned");
      return SF_ERR_ARG;
    }
    SF_FLUSH_VIEW(b, stream);
    if (stack_done)  // `current_obs *= masks` for the finished envs, then the new frame into its slot
      HIP_TRY(sf_launch_stack_clear(frames_dev - (size_t)stack_slot * frame, (size_t)stack_n * frame, stack_done, b->n_envs, stream));
    HIP_TRY(sf_launch_render_generic(b->d_state.get(), b->n_envs, b->g_w, b->g_h, b->g_sx, b->g_sy, b->g_vx, b->g_vy, b->g_lw,
                                     b->d_consts.get() + SF_LDS_TRIG, b->d_arcs.get(), b->d_gbg.get(), b->d_gtabs.get(), frames_dev, env_stride,
                                     mode == SF_OBS_IMAGE ? 1 : 0, b->d_glyphs.get(), stream));
    return SF_OK;
  }
  if (env_stride == 0) env_stride = frame;
  if (((uintptr_t)frames_dev & 15) != 0 || env_stride < frame || (env_stride & (mode == SF_OBS_IMAGE ? 15 : 7)) != 0) {
    sf_set_error("image frames must be 16-byte aligned, env_stride >= the frame size and a multiple of %d",
                 mode == SF_OBS_IMAGE ? 16 : 8);
    return SF_ERR_ARG;
  }
  SF_FLUSH_VIEW(b, stream);
  // first frame of a batch that steps with a symbolic observation: the caches, pictures and draw records (feature-only
  // batches never pay for them; image batches made them in sf_create)
  SF_TRY(sfb_ensure_render_resources(b, stream));
  // the state changed otherwise than through a step launch of an image batch: records from the state
  if (!b->draw_current) SF_TRY(sfb_rebuild_draw_records(b, stream));
  const PictureTail tail = picture_tail(b);
  unsigned char* const xcache = b->d_xcache.get();
  HIP_TRY(sf_launch_render(b->d_state.get(), b->d_draw.get(), b->n_envs, b->d_bg.get(), b->d_bg84.get(), b->d_tabs.get(), frames_dev, env_stride,
                           xcache, xcache ? xcache + tail.fort : nullptr, mode == SF_OBS_IMAGE ? 1 : 0, stack_done, stack_slot, stack_n,
                           stack_prev, b->args.hint, xcache ? xcache + tail.hud : nullptr, b->d_consts.get() + SF_LDS_TRIG, b->d_arcs.get(),
                           b->d_falpha.get(), b->d_glyphs.get(), stream));
  return SF_OK;
}

extern "C" int sf_draw_records(sf_batch* b, void* host, size_t bytes, int from_state) {
  static_assert(SF_DRAW_RECORD_BYTES == SF_DR_BYTES, "sfmi.h vs sf_drawrec.h");
  if (!b || !host || bytes != (size_t)b->n_envs * SF_DR_BYTES) {
    sf_set_error("sf_draw_records: need a batch and n_envs * %d bytes", SF_DR_BYTES);
    return SF_ERR_ARG;
  }
  DeviceGuard guard(b->device);
  HIP_TRY(hipDeviceSynchronize());
  if (from_state) {
    SF_FLUSH_VIEW(b, nullptr);
    SF_TRY(sfb_ensure_render_resources(b, nullptr));
    SF_TRY(sfb_rebuild_draw_records(b, nullptr));
  } else if (!b->d_draw) {
    sf_set_error("sf_draw_records: this batch has no draw records yet (they come with its first frame)");
    return SF_ERR_ARG;
  }
  // (the caller gets them env by env, whatever the device layout: sf_drawrec.h)
  std::vector<unsigned char> raw((size_t)b->args.lanes * SF_DR_BYTES);
  HIP_TRY(hipMemcpy(raw.data(), b->d_draw.get(), raw.size(), hipMemcpyDeviceToHost));
  for (long e = 0; e < b->n_envs; e++)  // (a record is contiguous: header, positions, headings)
    memcpy((unsigned char*)host + (size_t)e * SF_DR_BYTES, raw.data() + (size_t)(e >> 6) * SF_DR_TILE_BYTES + (size_t)(e & 63) * SF_DR_LANE_STRIDE,
           SF_DR_BYTES);
  return SF_OK;
}

extern "C" int sf_render(sf_batch* b, int mode, uint8_t* frames_dev, size_t env_stride, void* stream) {
  if (!b || !frames_dev) {
    sf_set_error("sf_render: null batch or output");
    return SF_ERR_ARG;
  }
  if (mode != SF_OBS_IMAGE && mode != SF_OBS_IMAGE_RAW) {
    sf_set_error("sf_render: mode must be SF_OBS_IMAGE or SF_OBS_IMAGE_RAW (got %d)", mode);
    return SF_ERR_ARG;
  }
  DeviceGuard guard(b->device);
  return sfb_render(b, mode, frames_dev, env_stride, (hipStream_t)stream);
}

extern "C" int sf_render_stack(sf_batch* b, uint8_t* stack_dev, int num_stack, int slot, const uint8_t* done_dev, void* stream) {
  if (!b || !stack_dev || num_stack < 1 || slot < 0 || slot >= num_stack) {
    sf_set_error("sf_render_stack: need a batch, the stack and 0 <= slot < num_stack");
    return SF_ERR_ARG;
  }
  DeviceGuard guard(b->device);
  const size_t frame = (size_t)SF_OUT * SF_OUT;
  return sfb_render(b, SF_OBS_IMAGE, stack_dev + (size_t)slot * frame, (size_t)num_stack * frame, (hipStream_t)stream, done_dev, slot,
                    num_stack);
}

extern "C" int sf_render_shift(sf_batch* b, const uint8_t* prev_stack_dev, uint8_t* stack_dev, int num_stack,
                               const uint8_t* done_dev, void* stream) {
  if (!b || !prev_stack_dev || !stack_dev || num_stack < 1 || ((uintptr_t)prev_stack_dev & 15) != 0) {
    sf_set_error("sf_render_shift: need a batch and two 16-byte aligned stacks");
    return SF_ERR_ARG;
  }
  const size_t frame = (size_t)SF_OUT * SF_OUT;
  {
    // an env's workgroup reads its own frames of the previous stack while others write theirs of the new one: the two
    // may touch (consecutive steps of a rollout's storage) but share no byte
    const uintptr_t p0 = (uintptr_t)prev_stack_dev, s0 = (uintptr_t)stack_dev;
    const size_t bytes = (size_t)b->n_envs * (size_t)num_stack * frame;
    if (p0 < s0 + bytes && s0 < p0 + bytes) {
      sf_set_error("sf_render_shift: the previous stack and the new one overlap");
      return SF_ERR_ARG;
    }
  }
  DeviceGuard guard(b->device);
  return sfb_render(b, SF_OBS_IMAGE, stack_dev + (size_t)(num_stack - 1) * frame, (size_t)num_stack * frame, (hipStream_t)stream,
                    done_dev, num_stack - 1, num_stack, prev_stack_dev);
}

extern "C" int sf_frame_stack_clear(uint8_t* stack_dev, size_t bytes_per_env, const uint8_t* done_dev, int n_envs, void* stream) {
  if (!stack_dev || !done_dev || n_envs <= 0 || (bytes_per_env & 15) != 0 || ((uintptr_t)stack_dev & 15) != 0) {
    sf_set_error("sf_frame_stack_clear: need 16-byte aligned stack, bytes_per_env a multiple of 16, done_dev, n_envs > 0");
    return SF_ERR_ARG;
  }
  HIP_TRY(sf_launch_stack_clear(stack_dev, bytes_per_env, done_dev, n_envs, (hipStream_t)stream));
  return SF_OK;
}

// ---- sf_render_view (sf_render_view.hip): frames in a view, for a range of lanes, from the state --------------------------------
namespace {
bool same_tables(const SfViewRes& a, const SfViewRes& b) {
  return a.w == b.w && a.h == b.h && a.sx == b.sx && a.sy == b.sy && a.vx == b.vx && a.vy == b.vy && a.lw == b.lw && a.band_h == b.band_h &&
         a.circle_k == b.circle_k && memcmp(&a.glyphs, &b.glyphs, sizeof(SfGlyphAtlas)) == 0;
}

// the batch's tables of view r: a cache entry, made on a miss (synchronous; an evicted entry's tables are freed only after the
// device has finished every frame that may read them).  A miss that fails leaves the entry empty.
int view_tables(sf_batch* b, const SfViewRes& r, const ViewCache** out) {
  int pick = 0;
  for (int i = 0; i < kViewCache; i++) {
    ViewCache& v = b->views[i];
    if (v.used && same_tables(v.res, r)) {
      v.used = ++b->view_clock;
      *out = &v;
      return SF_OK;
    }
    if (v.used < b->views[pick].used) pick = i;
  }
  std::vector<uint8_t> bg;
  std::vector<double> circle;
  size_t bg_stride = 0;
  SF_TRY(sf_view_tables(r, &bg, &bg_stride, &circle));
  ViewCache& v = b->views[pick];
  if (v.used) {
    HIP_TRY(hipDeviceSynchronize());  // (frames of the evicted view may still read its tables)
    v.d_bg.reset();
    v.d_circle.reset();
    v.used = 0;
  }
  DevBuf<uint8_t> nbg;
  DevBuf<double> ncircle;
  HIP_TRY(nbg.alloc(bg.size()));
  HIP_TRY(ncircle.alloc(circle.size()));
  if (!v.d_glyphs) HIP_TRY(v.d_glyphs.alloc(1));  // (an entry keeps its atlas buffer from view to view)
  HIP_TRY(hipMemcpy(nbg.get(), bg.data(), bg.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ncircle.get(), circle.data(), circle.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(v.d_glyphs.get(), &r.glyphs, sizeof(SfGlyphAtlas), hipMemcpyHostToDevice));
  v.d_bg = std::move(nbg);
  v.d_circle = std::move(ncircle);
  v.res = r;
  v.bg_stride = bg_stride;
  v.used = ++b->view_clock;
  *out = &v;
  return SF_OK;
}
}  // namespace

extern "C" int sf_view_size(const sf_batch* b, const sf_view* view, int32_t* width, int32_t* height) {
  if (!b) {
    sf_set_error("sf_view_size: null batch");
    return SF_ERR_ARG;
  }
  SfViewRes r;
  const int rc = sf_view_resolve(view, b->preset.width, b->preset.height, &r);
  if (rc != SF_OK) return rc;
  if (width) *width = r.w;
  if (height) *height = r.h;
  return SF_OK;
}

extern "C" int sf_render_view(sf_batch* b, const sf_view* view, int first_lane, int n_lanes, uint8_t* out_dev, size_t lane_stride,
                              void* stream) {
  if (!b) {
    sf_set_error("sf_render_view: null batch");
    return SF_ERR_ARG;
  }
  SfViewRes r;
  int rc = sf_view_resolve(view, b->preset.width, b->preset.height, &r);
  if (rc != SF_OK) return rc;
  if (first_lane < 0 || n_lanes < 0 || (long)first_lane + n_lanes > (long)b->n_envs) {
    sf_set_error("sf_render_view: lanes [%d, %d + %d) are not inside the batch's %d", first_lane, first_lane, n_lanes, b->n_envs);
    return SF_ERR_ARG;
  }
  const size_t frame = (size_t)r.w * r.h * (r.format == SF_VIEW_GRAY ? 1 : (r.format == SF_VIEW_RGB ? 3 : 4));
  if (lane_stride == 0) lane_stride = frame;
  if (!out_dev || lane_stride < frame) {
    sf_set_error("sf_render_view: need an output and a lane stride of at least the frame's %zu bytes", frame);
    return SF_ERR_ARG;
  }
  if (n_lanes == 0) return SF_OK;
  DeviceGuard guard(b->device);
  const ViewCache* tables = nullptr;
  rc = view_tables(b, r, &tables);
  if (rc != SF_OK) return rc;
  SF_FLUSH_VIEW(b, stream);
  const ViewCache& v = *tables;
  const SfViewLaunch L{b->d_state.get(), first_lane, n_lanes, r.w, r.h, r.band_h, r.planes, r.format, r.sx, r.sy, r.vx, r.vy, r.lw,
                       b->d_consts.get() + SF_LDS_TRIG, b->d_arcs.get(), v.d_circle.get(), r.circle_k, v.d_bg.get(), v.bg_stride,
                       v.d_glyphs.get(), out_dev, lane_stride};
  HIP_TRY(sf_launch_render_view(L, (hipStream_t)stream));
  return SF_OK;
}
