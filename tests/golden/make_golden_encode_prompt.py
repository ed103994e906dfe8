#!/usr/bin/env python3
"""Golden fixture of tests/test_oracle_text_encoders.py::test_oracle_matches_reference_encode_prompt, made by RUNNING THE
REFERENCE'S encode_prompt (adv_grpo/diffusers_patch/train_dreambooth_lora_sd3.py:98-144) on that test's own seeded transformers
modules (_models(3)).  Stored: the token ids (to show that the test rebuilt the same inputs) and the reference's outputs.
Usage: python tests/golden/make_golden_encode_prompt.py <reference checkout>"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_oracle_text_encoders import _models  # noqa: E402

sys.path.insert(0, os.path.abspath(sys.argv[1]))
from adv_grpo.diffusers_patch.train_dreambooth_lora_sd3 import encode_prompt  # noqa: E402

cl, cg, t5, ids, ids_t5 = _models(3)
with torch.no_grad():
    pe, pooled = encode_prompt([cl, cg, t5], [None, None, None], ["a", "b"], 40, device="cpu", text_input_ids_list=[ids, ids, ids_t5])
np.savez_compressed(os.path.join(HERE, "encode_prompt.npz"), ids=ids.numpy(), ids_t5=ids_t5.numpy(), prompt_embeds=pe.numpy(),
                    pooled=pooled.numpy())
print("wrote encode_prompt.npz", pe.shape, pooled.shape)
