"""Time the student generate() (evaluate_onevision.py:185-195 settings) on the real 0.5B student:
prefill of one 336x336 prompt (L = 1536) + 32 greedy decode steps with the KV cache.
    python tools/bench_generate.py
    python tools/bench_generate.py --batch 16    also generate_batch() at nb in {1, 2, 4, 8, 16} <= 16:
                                                 the batched step against the single-prompt step
                                                 measured in the same process
    python tools/bench_generate.py --grouped 6   also generate_grouped(): 16 prompts over ceil(16 / 6) images
                                                 (6 questions per image) against generate_batch() on the same
                                                 16 prompts, same process; --grouped 1: nothing is shared"""
import argparse
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd.data import synthetic_batch  # noqa
from knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd.generation import (  # noqa
    generate, generate_batch, generate_grouped)
from knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd.modeling import (  # noqa
    STUDENT_05B, LlavaOnevisionModel)

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=0, metavar="N",
                help="also time generate_batch() at every nb in {1, 2, 4, 8, 16} up to N")
ap.add_argument("--grouped", type=int, default=0, metavar="Q",
                help="also time generate_grouped() on 16 prompts, Q questions per image, against generate_batch()")
args = ap.parse_args()

dev = torch.device("cuda:0")
model = LlavaOnevisionModel(STUDENT_05B, dev, seed=2)
b = synthetic_batch(1, dev, L=1536, seed=0)
kw = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, eos_token_id=())


def best_of(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def timed(n_new):
    return best_of(lambda: generate(model, b["depth_input_ids"], b["depth_pixel_values"], b["image_sizes"],
                                    max_new_tokens=n_new, **kw))


t32, t96 = timed(32), timed(96)
t0 = time.perf_counter()
model.forward(b["depth_input_ids"], b["depth_pixel_values"], b["image_sizes"])
torch.cuda.synchronize()
pre = time.perf_counter() - t0
step1 = (t96 - t32) / 64 * 1e3
print(f"generate 0.5B student, 336x336 prompt (L=1536) + 32 tokens: {t32 * 1e3:.1f} ms per call "
      f"(prefill forward {pre * 1e3:.1f} ms); graph-replayed decode step {step1:.3f} ms/token "
      f"(marginal cost from 32 -> 96 new tokens)")

if args.batch > 0:
    # distinct 336x336 prompts (different seeds, L = 1536 each: every row's cache is as long as the
    # single-prompt run's); the marginal step cost from 32 -> 96 new tokens as above
    rows = [synthetic_batch(1, dev, L=1536, seed=s) for s in range(min(args.batch, 16))]
    prompts = [(r["depth_input_ids"], r["depth_pixel_values"], r["image_sizes"]) for r in rows]
    print(f"generate_batch, same process: single-prompt step {step1:.3f} ms/token")
    for nb in (1, 2, 4, 8, 16):
        if nb > args.batch:
            break
        tb = [best_of(lambda: generate_batch(model, prompts[:nb], max_new_tokens=n, **kw)) for n in (32, 96)]
        step = (tb[1] - tb[0]) / 64 * 1e3
        print(f"  nb={nb:2d}: {tb[0] * 1e3:7.1f} ms per call of 32 tokens; decode step {step:.3f} ms/step = "
              f"{step / nb:.3f} ms/token/row ({step / step1:.2f}x the single-prompt step, "
              f"{step1 * nb / step:.2f}x its tokens/s)")

if args.grouped > 0:
    # 16 prompts over ceil(16 / Q) synthetic 336x336 images, L = 1536 each: one synthetic_batch per image
    # (template head + image tokens), the 27 ids after the last image token redrawn per question
    from knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd.data import TEXT_VOCAB  # noqa
    from knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd.modeling import IMAGE_TOKEN_ID  # noqa
    Q, NP = args.grouped, 16
    groups, prompts = [], []
    for g0 in range(0, NP, Q):
        r = synthetic_batch(1, dev, L=1536, seed=100 + g0)
        ids = r["depth_input_ids"]
        P0 = int((ids[0] == IMAGE_TOKEN_ID).nonzero().max()) + 1
        qs = []
        for qi in range(g0, min(g0 + Q, NP)):
            gq = torch.Generator().manual_seed(1000 + qi)
            suf = torch.randint(0, TEXT_VOCAB, (1, 1536 - P0), generator=gq, dtype=torch.int64).to(dev)
            qs.append(torch.cat([ids[:, :P0], suf], 1))
        groups.append((r["depth_pixel_values"], r["image_sizes"], qs))
        prompts += [(q, r["depth_pixel_values"], r["image_sizes"]) for q in qs]
    print(f"generate_grouped, Q = {Q}: {NP} prompts over {len(groups)} images (L = 1536, {1536 - P0} tokens after "
          f"the image), against generate_batch on the same prompts, same process")
    for n in (32, 96):
        tg = best_of(lambda: generate_grouped(model, groups, max_new_tokens=n, **kw))
        tb = best_of(lambda: generate_batch(model, prompts, max_new_tokens=n, **kw))
        print(f"  {n:2d} new tokens: generate_grouped {tg * 1e3:7.1f} ms per call, generate_batch {tb * 1e3:7.1f} ms "
              f"per call, ratio {tg / tb:.3f} ({tb / tg:.2f}x)")
