/* contour_ref.c -- sequential CPU restatement of the reference's extracted_contour (my_function.cpp:8-145) for the
 * tests of bs_footprints: quantise + threshold, a separate dilation / erosion pass per iteration, Suzuki-Abe
 * border following with pixel marking (OpenCV's scanner and follower, full parent bookkeeping), contourArea,
 * arcLength and the OBJ writer.  Deliberately not the state-graph formulation of csrc/bs_contour.hip.
 * Built by the tests with `gcc -O2 -shared -fPIC -ffp-contract=off`; plain C, no dependencies. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* save_image (TMC3.cpp:100-108) + threshold (my_function.cpp:20): out[h][w] = 1 iff q > thr */
void ref_mask(const double* img, int w, int h, int thr, uint8_t* out)
{
  double max1 = 0;
  for (int64_t i = 0; i < (int64_t)w * h; i++)
    if (max1 < img[3 * i + 1])
      max1 = img[3 * i + 1];
  for (int64_t i = 0; i < (int64_t)w * h; i++) {
    int q = 0;
    if (max1 != 0) {
      const double t = 255.0 * (1.0 * img[3 * i + 1] / max1);
      q = t > 0 ? (int)(uint8_t)t : 0;
    }
    out[i] = q > thr;
  }
}

/* getStructuringElement(MORPH_ELLIPSE, Size(s, s)) */
void ref_ellipse(int s, uint8_t* k)
{
  const int r = s / 2, c = s / 2;
  const double inv_r2 = r ? 1. / ((double)r * r) : 0;
  memset(k, 0, (size_t)s * s);
  for (int i = 0; i < s; i++) {
    const int dy = i - r;
    int j1 = 0, j2 = 0;
    if (abs(dy) <= r) {
      const int dx = (int)lrint(c * sqrt((r * r - dy * dy) * inv_r2));
      j1 = c - dx > 0 ? c - dx : 0;
      j2 = c + dx + 1 < s ? c + dx + 1 : s;
    }
    for (int j = j1; j < j2; j++)
      k[i * s + j] = 1;
  }
}

static void morph_pass(const uint8_t* src, uint8_t* dst, int w, int h, const uint8_t* k, int s, int dilate)
{
  const int a = s / 2;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      uint8_t acc = dilate ? 0 : 1;
      for (int i = 0; i < s; i++)
        for (int j = 0; j < s; j++) {
          if (!k[i * s + j])
            continue;
          const int xx = x + j - a, yy = y + i - a;
          const uint8_t v = (xx < 0 || yy < 0 || xx >= w || yy >= h) ? (dilate ? 0 : 1) : src[(int64_t)yy * w + xx];
          if (dilate)
            acc |= v;
          else
            acc &= v;
        }
      dst[(int64_t)y * w + x] = acc;
    }
}

/* morphologyEx(MORPH_CLOSE, ellipse s x s, iterations): `iterations` dilations, then as many erosions, in place */
void ref_close(uint8_t* m, int w, int h, int s, int iterations)
{
  uint8_t* k = malloc((size_t)s * s);
  uint8_t* t = malloc((size_t)w * h);
  ref_ellipse(s, k);
  for (int it = 0; it < 2 * iterations; it++) {
    morph_pass(m, t, w, h, k, s, it < iterations);
    memcpy(m, t, (size_t)w * h);
  }
  free(t);
  free(k);
}

/* ---- findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) ---- */
static const int DX[8] = {1, 1, 0, -1, -1, -1, 0, 1};
static const int DY[8] = {0, -1, -1, -1, 0, 1, 1, 1};

typedef struct {
  int32_t* xy;
  int64_t n, cap;
} Pts;

static void push(Pts* p, int32_t x, int32_t y)
{
  if (p->n == p->cap) {
    p->cap = p->cap ? 2 * p->cap : 1024;
    p->xy = realloc(p->xy, (size_t)p->cap * 2 * sizeof(int32_t));
  }
  p->xy[2 * p->n] = x;
  p->xy[2 * p->n + 1] = y;
  p->n++;
}

typedef struct {
  int32_t n_contours;
  int64_t* offset;
  int32_t* xy;
  double* area;
  double* perimeter;
} RefContours;

/* Suzuki & Abe (1985), Algorithm 1, with OpenCV's search order and CHAIN_APPROX_SIMPLE emission; the mask m [h][w]
 * (0 / non-zero) is padded by a zero frame.  The outer borders whose parent is the frame are returned, in reverse
 * discovery order.  Returns 0, or -1 when memory runs out. */
int ref_find_contours(const uint8_t* m, int w, int h, RefContours* out)
{
  const int64_t wp = w + 2, hp = h + 2;
  int32_t* f = calloc((size_t)(wp * hp), sizeof(int32_t));
  int64_t bcap = 1024;
  uint8_t* is_hole = malloc(bcap);
  int32_t* parent = malloc(bcap * sizeof(int32_t));
  int64_t* starts = NULL;
  int64_t ncont = 0, ccap = 0;
  Pts pts = {0, 0, 0};
  if (!f || !is_hole || !parent)
    return -1;
  for (int64_t y = 0; y < h; y++)
    for (int64_t x = 0; x < w; x++)
      f[(y + 1) * wp + x + 1] = m[y * w + x] ? 1 : 0;
  int32_t nbd = 1;
  is_hole[1] = 1;  /* the frame counts as a hole border */
  parent[1] = 0;
  for (int64_t i = 1; i < hp - 1; i++) {
    int32_t lnbd = 1;
    for (int64_t j = 1; j < wp - 1; j++) {
      const int64_t p0 = i * wp + j;
      const int32_t v = f[p0];
      int hole;
      int s;
      if (v == 1 && f[p0 - 1] == 0) {
        hole = 0;
        s = 4;
      } else if (v >= 1 && f[p0 + 1] == 0) {
        hole = 1;
        s = 0;
        if (v > 1)
          lnbd = v;
      } else {
        if (v != 0 && v != 1)
          lnbd = v < 0 ? -v : v;
        continue;
      }
      nbd++;
      if (nbd >= bcap) {
        bcap *= 2;
        is_hole = realloc(is_hole, bcap);
        parent = realloc(parent, bcap * sizeof(int32_t));
      }
      is_hole[nbd] = (uint8_t)hole;
      /* Table 1 */
      if (hole == is_hole[lnbd])
        parent[nbd] = parent[lnbd];
      else
        parent[nbd] = lnbd;
      const int keep = !hole && parent[nbd] == 1;
      const int64_t pstart = pts.n;
      /* (3.1) clockwise from (i2, j2) */
      const int s_end0 = s;
      int64_t i1 = -1;
      do {
        s = (s - 1) & 7;
        const int64_t q = p0 + DY[s] * wp + DX[s];
        if (f[q] != 0) {
          i1 = q;
          break;
        }
      } while (s != s_end0);
      if (i1 < 0) {
        f[p0] = -nbd;
        if (keep)
          push(&pts, (int32_t)(j - 1), (int32_t)(i - 1));
      } else {
        int64_t i3 = p0;
        int prev_s = s ^ 4;
        for (;;) {
          int east_zero = 0;
          int64_t i4;
          for (;;) { /* (3.3) counter-clockwise from the element after (i2, j2) */
            s = (s + 1) & 7;
            i4 = i3 + DY[s] * wp + DX[s];
            if (f[i4] != 0)
              break;
            if (s == 0)
              east_zero = 1;
          }
          if (east_zero) /* (3.4) */
            f[i3] = -nbd;
          else if (f[i3] == 1)
            f[i3] = nbd;
          if (s != prev_s) {
            if (keep)
              push(&pts, (int32_t)(i3 % wp - 1), (int32_t)(i3 / wp - 1));
            prev_s = s;
          }
          if (i4 == p0 && i3 == i1) /* (3.5) */
            break;
          i3 = i4;
          s = (s + 4) & 7;
        }
      }
      if (keep) {
        if (ncont + 1 >= ccap) {
          ccap = ccap ? 2 * ccap : 256;
          starts = realloc(starts, ccap * sizeof(int64_t));
        }
        starts[ncont++] = pstart;
      }
      /* (4) */
      if (f[p0] != 1)
        lnbd = f[p0] < 0 ? -f[p0] : f[p0];
    }
  }
  /* reverse discovery order (cvInsertNodeIntoTree prepends) */
  out->n_contours = (int32_t)ncont;
  out->offset = malloc((ncont + 1) * sizeof(int64_t));
  out->xy = malloc((pts.n ? pts.n : 1) * 2 * sizeof(int32_t));
  out->area = malloc((ncont ? ncont : 1) * sizeof(double));
  out->perimeter = malloc((ncont ? ncont : 1) * sizeof(double));
  int64_t o = 0;
  out->offset[0] = 0;
  for (int64_t c = 0; c < ncont; c++) {
    const int64_t src = ncont - 1 - c;
    const int64_t a = starts[src], e = src + 1 < ncont ? starts[src + 1] : pts.n;
    memcpy(out->xy + 2 * o, pts.xy + 2 * a, (size_t)(e - a) * 2 * sizeof(int32_t));
    const int32_t* P = out->xy + 2 * o;
    const int64_t n = e - a;
    /* contourArea (oriented = false) */
    double a00 = 0;
    double px = P[2 * (n - 1)], py = P[2 * (n - 1) + 1];
    for (int64_t k = 0; k < n; k++) {
      const double x = P[2 * k], y = P[2 * k + 1];
      a00 += px * y - py * x;
      px = x;
      py = y;
    }
    out->area[c] = fabs(a00 * 0.5);
    /* arcLength(closed = true) */
    double per = 0;
    float fx = (float)P[2 * (n - 1)], fy = (float)P[2 * (n - 1) + 1];
    for (int64_t k = 0; k < n; k++) {
      const float x = (float)P[2 * k], y = (float)P[2 * k + 1];
      const float dx = x - fx, dy = y - fy;
      per += sqrtf(dx * dx + dy * dy);
      fx = x;
      fy = y;
    }
    out->perimeter[c] = per;
    o += n;
    out->offset[c + 1] = o;
  }
  free(pts.xy);
  free(starts);
  free(parent);
  free(is_hole);
  free(f);
  return 0;
}

void ref_contours_free(RefContours* c)
{
  free(c->offset);
  free(c->xy);
  free(c->area);
  free(c->perimeter);
  memset(c, 0, sizeof *c);
}

/* the OBJ loop of my_function.cpp:64-131 (ASCII captions) */
int ref_write_obj(const RefContours* c, int w, int h, const char* path)
{
  FILE* f = fopen(path, "w");
  if (!f)
    return -1;
  fprintf(f, "# building footprints extruded to a 3-D model\n");
  fprintf(f, "# contours: %d\n", c->n_contours);
  fprintf(f, "# x, y normalised to [0,1]\n\n");
  for (int32_t i = 0; i < c->n_contours; i++)
    for (int64_t k = c->offset[i]; k < c->offset[i + 1]; k++) {
      const float x = (float)c->xy[2 * k] / w;
      const float y = 1.0f - (float)c->xy[2 * k + 1] / h;
      fprintf(f, "v %g %g 0.0\n", x, y);
      fprintf(f, "v %g %g %d\n", x, y, 1);
    }
  fprintf(f, "\n# faces (quads)\n");
  int64_t vi = 1;
  for (int32_t i = 0; i < c->n_contours; i++) {
    const int64_t n = c->offset[i + 1] - c->offset[i];
    for (int64_t k = 0; k < n; k++) {
      const int64_t nx = (k + 1) % n;
      fprintf(f, "f %lld %lld %lld %lld\n", (long long)(vi + 2 * k), (long long)(vi + 2 * nx),
              (long long)(vi + 2 * nx + 1), (long long)(vi + 2 * k + 1));
    }
    vi += 2 * n;
  }
  return fclose(f);
}

/* the whole stage: image [h][w][3] f64 -> closed mask (0 / 1, nullable) and contours */
int ref_footprints(const double* img, int w, int h, int thr, int ks, int iterations, uint8_t* mask_out,
                   RefContours* out)
{
  uint8_t* m = malloc((size_t)w * h);
  if (!m)
    return -1;
  ref_mask(img, w, h, thr, m);
  if (iterations > 0)
    ref_close(m, w, h, ks, iterations);
  if (mask_out)
    memcpy(mask_out, m, (size_t)w * h);
  const int rc = ref_find_contours(m, w, h, out);
  free(m);
  return rc;
}
