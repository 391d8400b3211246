# Databricks notebook source
# MAGIC %md
# MAGIC ## BERT-large pretraining: masked LM + next-sentence prediction, seq 512, LAMB
# MAGIC
# MAGIC The `bert_large_lamb` harness on its pretraining objective.  Each sequence carries 76 masked
# MAGIC positions (`mlm_predictions`); only those rows are gathered and run through the MLM head, and
# MAGIC the vocabulary projection (tied to the word embedding) and its loss are one fused op
# MAGIC (`ops.linear_cross_entropy`): the `[rows, 30522]` logits exist once and their gradient
# MAGIC overwrites them.  `batch_size=0` sizes the micro-batch for the HBM of one MI355X.

# COMMAND ----------

import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__) if "__file__" in dir() else ".", "../..")))

import torch

from databricks_distributed_deep_learning_amd import get_preset
from databricks_distributed_deep_learning_amd.parallel import Distributor
from databricks_distributed_deep_learning_amd.training import train

SMOKE = os.environ.get("DDL_NOTEBOOK_SMOKE") == "1"

# COMMAND ----------

if SMOKE or not torch.cuda.is_available():
    cfg = get_preset("bert_large_pretrain", batch_size=1, seq_len=16, mlm_predictions=3, steps=1, warmup_steps=0,
                     grad_accum=2, dtype="fp32", backend="gloo", native="off")
    n, gpu = 1, False
else:
    cfg = get_preset("bert_large_pretrain", steps=10, warmup_steps=2)
    n, gpu = torch.cuda.device_count(), True
if __name__ == "__main__":
    print(Distributor(num_processes=n, use_gpu=gpu).run(train, cfg))
