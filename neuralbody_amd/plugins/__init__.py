"""Plugin files for the reference's `imp.load_source(cfg.X_module, cfg.X_path)` factories
(lib/networks/make_network.py:5-9, lib/networks/renderer/make_renderer.py:5-9,
lib/train/trainers/make_trainer.py:5-14).  Select them from the command line, e.g.

    python run.py --type visualize --cfg_file configs/zju_mocap_exp/latent_xyzc_313.yaml \
        network_path /path/to/neuralbody_amd/plugins/latent_xyzc.py \
        renderer_path /path/to/neuralbody_amd/plugins/if_clight_renderer.py \
        trainer_path /path/to/neuralbody_amd/plugins/if_nerf_clight.py

The training dataset goes through `imp.load_source(cfg.train_dataset_module, cfg.train_dataset_path)` too
(lib/datasets/make_dataset.py:13-23); it draws its rays on the device, so it runs in the training process:

    python train_net.py --cfg_file configs/zju_mocap_exp/latent_xyzc_313.yaml exp_name xyzc_313 resume False \
        train_dataset_path /path/to/neuralbody_amd/plugins/light_stage_dataset.py train.num_workers 0 \
        network_path ... renderer_path ... trainer_path ...
"""
