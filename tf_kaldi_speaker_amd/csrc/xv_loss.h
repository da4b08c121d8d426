#pragma once
#include "xv_common.h"

// xv_margin_softmax_rows in one launch (mean folded in through a ticket) that also writes ||x[r]|| (xv_loss.hip)
int xv_margin_softmax_rows_ex(hipStream_t s, int kind, const float* logits, int rows, int n, int ldl, const float* x, int c,
                              const int32_t* labels, float m, float lambda, float* dlogits, float* dnorm, float* row_loss,
                              float* loss_out, float* xnorm, uint32_t* ticket);
