// The host-side argument checks of csrc/prpp.hip as a stand-alone program for a sanitizer build on a machine without a GPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         smilecode_amd/csrc/prpp.hip -x hip tools/micro/prpp_refusals.cpp -o /tmp/prpp_refusals && /tmp/prpp_refusals
//
// Every call below is refused before its first launch (NULL pointers, counts below 1, channel counts outside the kernels',
// misaligned tensors, a short or misaligned workspace), so nothing is launched and no device is needed; the "device" pointers are
// host addresses that are never dereferenced.  Prints one line per group and returns the number of wrong answers.
#include <stdint.h>
#include <stdio.h>

#include "../../include/modet_hip_prpp.h"

static int bad = 0;
#define EXPECT(call, code) do { const int rc_ = (call); if (rc_ != (code)) { printf("line %d: %s = %d, expected %d\n", __LINE__, #call, rc_, (code)); ++bad; } } while (0)

int main(void) {
  alignas(64) static float buf[4096];
  float* a = buf;                      // 64-byte aligned
  float* a4 = buf + 1;                 // 4-byte aligned only
  float* a2 = (float*)((char*)buf + 2);
  void* ws = buf + 1024;

  EXPECT(modet_prpp_upcat_fwd(nullptr, a, a, 1, 2, 2, 2, 4, 4, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_upcat_fwd(a, nullptr, a, 1, 2, 2, 2, 4, 4, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_upcat_fwd(a, a, nullptr, 1, 2, 2, 2, 4, 4, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_upcat_fwd(a, a, a, 0, 2, 2, 2, 4, 4, nullptr), MODET_ERR_DIM);
  EXPECT(modet_prpp_upcat_fwd(a, a, a, 1, 2, 0, 2, 4, 4, nullptr), MODET_ERR_DIM);
  EXPECT(modet_prpp_upcat_fwd(a, a, a, 1, 2, 2, 2, 0, 4, nullptr), MODET_ERR_DIM);
  EXPECT(modet_prpp_upcat_fwd(a, a, a2, 1, 2, 2, 2, 4, 4, nullptr), MODET_ERR_UNSUPPORTED);
  EXPECT(modet_prpp_upcat_bwd(a, nullptr, nullptr, 1, 2, 2, 2, 4, 4, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_upcat_bwd(nullptr, a, a, 1, 2, 2, 2, 4, 4, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_upcat_bwd(a, a, a, 1, 2, 2, -1, 4, 4, nullptr), MODET_ERR_DIM);
  printf("upcat: checked\n");

  EXPECT(modet_prpp_relu_fwd(nullptr, a, 8, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_relu_fwd(a, nullptr, 8, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_relu_fwd(a, a, 0, nullptr), MODET_ERR_DIM);
  EXPECT(modet_prpp_relu_fwd(a4, a, 8, nullptr), MODET_ERR_UNSUPPORTED);
  EXPECT(modet_prpp_relu_add_fwd(nullptr, a, a, 8, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_relu_add_fwd(a, a, a4, 8, nullptr), MODET_ERR_UNSUPPORTED);
  EXPECT(modet_prpp_relu_bwd(a, nullptr, a, 8, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_relu_bwd(a, a, a, -3, nullptr), MODET_ERR_DIM);
  printf("relu: checked\n");

  const size_t nb = modet_prpp_stack_ws_bytes(1, 2, 3, 4, 8);
  EXPECT((int)(nb == 2 * (2 * 3 * 4 * 8 + 4 * 5 * 6 * 8) * sizeof(float)), 1);
  EXPECT((int)modet_prpp_stack_ws_bytes(1, 2, 3, 4, 6), 0);
  EXPECT((int)modet_prpp_stack_ws_bytes(1, 2, 3, 4, MODET_PRPP_MAX_C + 4), 0);
  EXPECT((int)modet_prpp_stack_ws_bytes(0, 2, 3, 4, 8), 0);
  EXPECT(modet_prpp_stack_fwd(nullptr, a, a, ws, nb, 1, 2, 3, 4, 8, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_stack_fwd(a, a, a, nullptr, nb, 1, 2, 3, 4, 8, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_stack_fwd(a, a, a, ws, nb - 1, 1, 2, 3, 4, 8, nullptr), MODET_ERR_WORKSPACE);
  EXPECT(modet_prpp_stack_fwd(a, a, a, (char*)ws + 4, nb, 1, 2, 3, 4, 8, nullptr), MODET_ERR_WORKSPACE);
  EXPECT(modet_prpp_stack_fwd(a, a, a, ws, nb, 1, 2, 3, 4, 6, nullptr), MODET_ERR_UNSUPPORTED);
  EXPECT(modet_prpp_stack_fwd(a, a, a, ws, nb, 1, 2, 3, 4, 132, nullptr), MODET_ERR_UNSUPPORTED);
  EXPECT(modet_prpp_stack_fwd(a, a, a, ws, nb, 1, 0, 3, 4, 8, nullptr), MODET_ERR_DIM);
  EXPECT(modet_prpp_stack_fwd(a4, a, a, ws, nb, 1, 2, 3, 4, 8, nullptr), MODET_ERR_UNSUPPORTED);
  EXPECT(modet_prpp_stack_bwd(a, a, a, nullptr, nullptr, ws, nb, 1, 2, 3, 4, 8, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_stack_bwd(a, a, nullptr, a, a, ws, nb, 1, 2, 3, 4, 8, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_stack_bwd(a, a, a, a, nullptr, ws, 0, 1, 2, 3, 4, 8, nullptr), MODET_ERR_WORKSPACE);
  EXPECT(modet_prpp_stack_bwd(a, a, a, a4, nullptr, ws, nb, 1, 2, 3, 4, 8, nullptr), MODET_ERR_UNSUPPORTED);
  printf("stack: checked\n");

  const size_t nc = modet_prpp_compose_ws_bytes(2, 2, 3, 5);
  EXPECT((int)(nc == 64 + 2 * 2 * 3 * 5 * 3 * 8), 1);
  EXPECT((int)modet_prpp_compose_ws_bytes(0, 2, 3, 5), 0);
  EXPECT((int)modet_prpp_compose_ws_bytes(2, 2, 0, 5), 0);
  EXPECT(modet_prpp_compose_fwd(nullptr, a, a, 2, 2, 3, 5, 4, 6, 10, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_compose_fwd(a, a, nullptr, 2, 2, 3, 5, 4, 6, 10, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_compose_fwd(a, a, a, 0, 2, 3, 5, 4, 6, 10, nullptr), MODET_ERR_DIM);
  EXPECT(modet_prpp_compose_fwd(a, a, a, 2, 2, 3, 5, 4, 1, 10, nullptr), MODET_ERR_DIM);
  EXPECT(modet_prpp_compose_fwd(a, a, a, 2, 0, 3, 5, 4, 6, 10, nullptr), MODET_ERR_DIM);
  EXPECT(modet_prpp_compose_fwd(a, a2, a, 2, 2, 3, 5, 4, 6, 10, nullptr), MODET_ERR_UNSUPPORTED);
  EXPECT(modet_prpp_compose_bwd(a, a, a, nullptr, nullptr, ws, nc, 2, 2, 3, 5, 4, 6, 10, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_compose_bwd(a, a, a, a, a, nullptr, nc, 2, 2, 3, 5, 4, 6, 10, nullptr), MODET_ERR_NULL);
  EXPECT(modet_prpp_compose_bwd(a, a, a, a, a, ws, nc - 1, 2, 2, 3, 5, 4, 6, 10, nullptr), MODET_ERR_WORKSPACE);
  EXPECT(modet_prpp_compose_bwd(a, a, a, a, a, (char*)ws + 8, nc, 2, 2, 3, 5, 4, 6, 10, nullptr), MODET_ERR_WORKSPACE);
  EXPECT(modet_prpp_compose_bwd(a, a, a, a, a, ws, nc, 2, 2, 3, 5, 1, 6, 10, nullptr), MODET_ERR_DIM);
  printf("compose: checked\n");

  printf("%d wrong answers\n", bad);
  return bad;
}
