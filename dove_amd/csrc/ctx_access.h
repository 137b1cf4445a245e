// What csrc/video.hip (the whole-video session) reads of a dove_ctx, whose layout is private to csrc/graph.hip.
#pragma once
#include "../../include/dove_hip.h"

const dove_model_config* dove_ctx_config(const dove_ctx* c);   // NULL until dove_finalize_weights has run
int dove_ctx_nranks(const dove_ctx* c);
int dove_ctx_device(const dove_ctx* c);
// make the context's arena large enough for a [3,F,H,W] dove_sr_clip now (dove_workspace_bytes; a caller-lent workspace is left as it is)
int dove_ctx_reserve(dove_ctx* c, int F, int H, int W);
