"""Shared defaults of the Stage-3 configs.  Keys and meanings are the reference's (train.py:41-90):
a config module exposes ``configurations = {1: dict(...)}`` and the driver reads ``configurations[1]``."""
import os

import numpy as np
import torch


def stage3(exp_name, **overrides):
    cfg = dict(
        SEED=900,
        EXP_NAME=exp_name,
        DATA_ROOT="<path to the folder containing BUPT-BalancedFace and test datasets as subfolders>",
        TRAIN_IMAGES_FOLDER="bupt-balancedface",
        MODEL_ROOT=os.path.join("exps/model/", exp_name),
        LOG_ROOT=os.path.join("exps/log", exp_name),
        BACKBONE_RESUME_ROOT="",
        HEAD_RESUME_ROOT="",
        OPTIMIZER_RESUME_ROOT="",
        BACKBONE_NAME="IR_50_ReStyle",   # pSp IR-SE-50 trunk, with or without a Stage-2 encoder checkpoint
        HEAD_NAME="ArcFace",             # ArcFace | CosFace | SphereFace | Am_softmax | CurricularFace | MagFace | AdaCos | NPCFace
                                         # | MV_Softmax (MV_IS_AM=True: additive margin, the default; False: ArcFace-style)
                                         # | CircleLoss | AM_Softmax (the FaceX-Zoo head; not Am_softmax) | ArcNegFace
                                         # | Softmax (the plain linear head with a bias)
        LOSS_NAME="Focal",               # Focal | Softmax (nn.CrossEntropyLoss(): the batch-mean cross entropy, on the HIP path)
        # optional, read by train.py when present: SHARDED_HEAD=True (the class-sharded head, frhip/sharded_head.py) and
        # with it SHARDED_HEAD_SAMPLE_RATE in (0, 1], default 1.0: below 1 a training step runs on that fraction of each
        # rank's classes, the classes of the batch among them, drawn from (SEED, batch counter); ArcFace, CosFace,
        # SphereFace and Softmax only, and the rate must keep at least min(classes per rank, global batch) classes.
        # SHARDED_HEAD_SPARSE_UPDATE=True (default False; needs SHARDED_HEAD=True, a rate below 1 and OPTIMIZER_NAME 'SGD'):
        # the optimizer updates only the sampled rows of the head and of its momentum; unselected rows see no weight decay
        # and no momentum step (the lazy update of Partial-FC v1), and no gradient of the head's full shape is formed
        ENCODER_CHECKPOINT=None,
        ENCODER_AVG_IMAGE="<an arbitrary 112x112 image here>",
        ENCODER_INPUT_SIZE=112,
        ENCODER_ADDITIONAL_DROPOUT=0.15,
        INPUT_SIZE=[112, 112],
        RGB_MEAN=[0.5, 0.5, 0.5],
        RGB_STD=[0.5, 0.5, 0.5],
        EMBEDDING_SIZE=512,
        BATCH_SIZE=100,                  # reference: global batch of nn.DataParallel; here: per process (= per GPU)
        DROP_LAST=True,
        FREEZE_BACKBONE_EPOCHS=3,
        LR=0.03,
        NUM_EPOCH=100,
        WEIGHT_DECAY=2e-3,               # not applied to batch-norm parameters
        MOMENTUM=0.9,
        GRAD_CLIP_NORM=None,             # a number > 0: clip the global L2 norm of the backbone's gradients to it every step
        SKIP_NONFINITE_STEP=False,       # True: a step whose backbone gradients hold an inf or a NaN updates nothing
                                         # (both on the device, frhip.optim.GradGuard; off: no launch is added)
        STAGES=np.arange(10, 125, 5) + 5,
        WARMUP=False,
        LAYER_DECAY=None,
        DEVICE=torch.device("cuda:0" if torch.cuda.is_available() else "cpu"),
        MULTI_GPU=True,
        GPU_ID=[0],
        PIN_MEMORY=True,
        NUM_WORKERS=8,
        GPU_RESIDENT_DATASET=False,      # True (needs GPU_INPUT_PIPELINE=True): decode the training set once into device
                                         # memory and draw every batch from there in one launch (frhip/resident.py); the
                                         # samples, crops, flips and checkpoints of the GPU_INPUT_PIPELINE run, bit for bit
        GPU_RESIDENT_MAX_GB=None,        # the most the resident set may take; None: half of the device's free memory
        GPU_RANDAUGMENT=False,           # True (needs GPU_INPUT_PIPELINE=True): the reference's Rand_Augment policy on the
                                         # decoded images, one more launch per batch (fr_randaug_u8); rotate, shearX, shearY
                                         # and sharpness are not served on the device
        GPU_RANDAUGMENT_NUM=None,        # operations per image, 1..16; None: half the number of operations (5 of 10)
        GPU_RANDAUGMENT_MAX_MAGNITUDE=10,  # magnitude indices are drawn below it, 1..10
        GPU_RANDAUGMENT_OPS=None,        # None: the served set (frhip.input_pipeline.SERVED), or a list of its names
    )
    cfg.update(overrides)
    return cfg
