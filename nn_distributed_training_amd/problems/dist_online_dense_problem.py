"""Online (streaming) implicit-density problem with a dynamic graph.

Capability parity with the reference's
``problems/dist_online_dense_problem.py``: per-node sliding-window lidar
datasets, a communication graph recomputed EVERY round from current robot
positions (euclidean disk graph with ``comm_radius``), a train-loss EMA
tracker, NaN guard, and optional model-state checkpointing.

Distributed design: robot positions are tiny ([N, 2]), so ``update_graph``
all-gathers positions each round and every rank re-derives the same
adjacency (and therefore the same P2P schedule) host-side — the schedule
stays deterministic without any negotiation.
"""

from __future__ import annotations

import copy
import os

import numpy as np
import torch

from ..utils import graph_generation
from .base import ProblemBase


class DistOnlineDensityProblem(ProblemBase):
    def __init__(self, base_model, base_loss, train_sets, val_set, device,
                 conf):
        self.comm_radius = conf["comm_radius"]
        self.dynamic_graph = conf["dynamic_graph"]
        N = len(train_sets)
        # build an initial graph before ProblemBase wires the comm layer:
        # all ranks hold all train_sets (data gen is seeded + cheap), so
        # initial positions are known everywhere.
        poses = np.vstack(
            [train_sets[i].curr_pos.reshape(1, 2) for i in range(N)]
        )
        graph, connected = graph_generation.euclidean_disk_graph(
            poses, self.comm_radius
        )
        if not connected:
            print("** WARNING: the communication graph is not connected. **")

        super().__init__(
            graph, base_model, base_loss, train_sets, val_set, device, conf
        )

        self.track_tloss = "train_loss_moving_average" in self.metrics
        if self.track_tloss:
            self.tloss_tracker = torch.zeros(self.N)
            self.tloss_decay = conf["metrics_config"]["tloss_decay"]

        if "mesh_grid_density" in self.metrics:
            X, Y = np.meshgrid(val_set.lidar.xs, val_set.lidar.ys)
            mesh = np.stack(
                [X[::8, ::8].reshape(-1), Y[::8, ::8].reshape(-1)], axis=1
            )
            self.mesh_inputs = torch.as_tensor(
                mesh, dtype=torch.get_default_dtype()
            ).to(self.device)
            self.metrics["mesh_inputs"] = self.mesh_inputs.cpu()

    # ------------------------------------------------------------------
    def local_batch_loss(self, i):
        locs, dens = self.next_batch(i)
        yh = self.models[i].forward(locs.to(self.device))
        if torch.isnan(yh).any():
            raise NameError(
                f"NaN forward output at node {i} "
                f"(param norm "
                f"{torch.nn.utils.parameters_to_vector(self.models[i].parameters()).norm():.3e})"
            )
        batch_loss = self.base_loss(torch.squeeze(yh), dens.to(self.device))
        if self.track_tloss:
            with torch.no_grad():
                if self.tloss_tracker[i] != 0.0:
                    self.tloss_tracker[i] *= 1 - self.tloss_decay
                    self.tloss_tracker[i] += (
                        self.tloss_decay * batch_loss.detach().cpu()
                    )
                else:
                    self.tloss_tracker[i] += batch_loss.detach().cpu()
        return batch_loss

    # ------------------------------------------------------------------
    def current_positions(self) -> np.ndarray:
        """All-node positions [N, 2]: local window positions all-gathered."""
        local_np = np.vstack(
            [
                self.train_sets[i].curr_pos.reshape(1, 2)
                for i in self.local_nodes
            ]
        )
        if self.comm.world == 1:
            # no device round-trip: the H2D/D2H pair costs a stream sync
            # every round (measured 16 ms/round on the density bench)
            return local_np
        local = torch.as_tensor(local_np, dtype=torch.float64).to(
            self.device
        )
        full = self.comm.all_gather_rows(self.layout, local)
        return full.cpu().numpy()

    def update_graph(self):
        """Re-derive the disk graph from current robot positions.

        Called once per communication round by the optimizers; in
        multi-rank mode every rank computes the identical graph from the
        all-gathered positions, keeping the P2P schedule deterministic.
        """
        if not self.dynamic_graph:
            return
        poses = self.current_positions()
        self.graph, connected = graph_generation.euclidean_disk_graph(
            poses, self.comm_radius
        )
        if not connected:
            self._print(
                "** WARNING: the communication graph is not connected. **"
            )

    # ------------------------------------------------------------------
    def save_metrics(self, output_dir):
        super().save_metrics(output_dir)
        if self.conf.get("save_models", False):
            if self.stacked is not None:
                self.stacked.flush_to_models()
            # every rank writes its local nodes' states; rank 0 keeps
            # the reference's file name (single-rank = all nodes there),
            # other ranks add per-rank shards
            state_dicts = {
                i: self.models[i].state_dict() for i in self.local_nodes
            }
            if self.is_root:
                file_name = self.conf["problem_name"] + "_models.pt"
            else:
                file_name = (
                    f"{self.conf['problem_name']}_models_rank"
                    f"{self.comm.rank}.pt"
                )
            torch.save(state_dicts, os.path.join(output_dir, file_name))

    # ------------------------------------------------------------------
    def validate(self, i):
        val_loss = 0.0
        with torch.no_grad():
            for locs, dens in self.val_loader:
                locs = locs.to(self.device)
                dens = dens.to(self.device)
                yh = self.models[i].forward(locs)
                val_loss += self.base_loss(torch.squeeze(yh), dens).item()
        return val_loss

    def mesh_grid_density(self, i):
        with torch.no_grad():
            return self.models[i].forward(self.mesh_inputs)

    # ------------------------------------------------------------------
    def evaluate_metrics(self, at_end=False):
        if self.stacked is not None:
            self.stacked.flush_to_models()
        evalprint = "| "
        for met_name in self.conf["metrics"]:
            if met_name == "consensus_error":
                distances_all, distances_mean = self.consensus_error()
                self.metrics[met_name].append(
                    (distances_all, distances_mean)
                )
                evalprint += "Consensus: {:.4f} - {:.4f} | ".format(
                    distances_mean.amin().item(),
                    distances_mean.amax().item(),
                )
            elif met_name == "validation_loss":
                if self.stacked is not None:
                    vl = self.stacked.validate_all()
                else:
                    vl = torch.tensor(
                        [self.validate(i) for i in self.local_nodes]
                    )
                val_losses = self.gather_per_node(vl)
                self.metrics[met_name].append(val_losses)
                evalprint += "Val Loss: {:.4f} - {:.4f} - {:.4f} | ".format(
                    val_losses.amin().item(),
                    val_losses.mean().item(),
                    val_losses.amax().item(),
                )
            elif met_name == "train_loss_moving_average":
                if self.stacked is not None and \
                        self.stacked.tloss_dev is not None:
                    self.tloss_tracker[self.local_nodes] = \
                        self.stacked.tloss_dev.cpu().to(
                            self.tloss_tracker.dtype
                        )
                tl = self.gather_per_node(
                    self.tloss_tracker[self.local_nodes]
                )
                self.metrics[met_name].append(tl.clone())
                evalprint += "Train Loss MA: {:.4f} - {:.4f} | ".format(
                    tl.amin().item(), tl.amax().item()
                )
            elif met_name == "mesh_grid_density":
                mc = self.conf["metrics_config"]
                if (not mc.get("mesh_only_at_end", False)) or at_end:
                    loc = self.mesh_grid_density_all()
                    if loc is None:
                        dens = [
                            self.mesh_grid_density(i)
                            for i in self.local_nodes
                        ]
                        loc = (
                            torch.stack(dens)
                            if dens
                            else torch.zeros(
                                0, *self.mesh_inputs.shape[:1], 1,
                                device=self.device,
                            )
                        )
                    # gather so rank 0 (the saver) has every node's mesh
                    self.metrics[met_name].append(
                        self.gather_per_node_rows(loc)
                    )
            elif met_name == "forward_pass_count":
                self.metrics[met_name].append(self.forward_cnt)
                evalprint += "Num Forward: {} | ".format(self.forward_cnt)
            elif met_name == "current_epoch":
                ep = self.gather_per_node(
                    self.epoch_tracker[self.local_nodes]
                )
                self.metrics[met_name].append(copy.deepcopy(ep))
                evalprint += "Ep Range: {} - {} | ".format(
                    int(ep.amin().item()), int(ep.amax().item())
                )
            elif met_name == "current_position":
                self.metrics[met_name].append(self.current_positions())
            elif met_name == "current_graph":
                self.metrics[met_name].append(copy.deepcopy(self.graph))
            else:
                raise NameError("Unknown metric.")
        self._print(evalprint)
